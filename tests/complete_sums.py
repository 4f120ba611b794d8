"""Complete sums (include/sbn.h, "Complete sums"): batches of short MSMs on the two curve tables whose starts the library picks
from its eight start candidates.  Shared by test_complete_sums_host.py and test_complete_sums_gpu.py.

Python integers are the reference, never the code under test: the candidates are re-derived here from their rule, the choice of
every segment is the smallest candidate from which Python's own walk of the segment (chained_lists.derive / walk_all) meets no
bad event, and every recipe asserts on the CPU that the kills it is meant to hold really kill the candidates it names."""
import functools

import numpy as np

import chained_lists as CL
import msm_batches as MB
import oracle_lib as O
import tracegen_edges as T

P, R = T.P, T.R
CANDIDATES = 8
GEN = CL.START


# ---------------------------------------------------------------- the candidates, from their rule
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = _f2mul(r, a)
        a = _f2mul(a, a)
        e >>= 1
    return r


def _f2sqrt(a):
    """A square root of a != 0 in Fq2 = Fq[i] / (i^2 + 1), or None (p = 3 mod 4: a1 = a^((p-3)/4), alpha = a1^2 a, x0 = a1 a; alpha
    = -1: i x0, else (1 + alpha)^((p-1)/2) x0)."""
    a1 = _f2pow(a, (P - 3) // 4)
    alpha, x0 = _f2mul(_f2mul(a1, a1), a), _f2mul(a1, a)
    r = _f2mul((0, 1), x0) if alpha == (P - 1, 0) else _f2mul(_f2pow(((1 + alpha[0]) % P, alpha[1]), (P - 1) // 2), x0)
    return r if _f2mul(r, r) == a else None


@functools.lru_cache(maxsize=None)
def candidates(curve):
    """The eight start candidates of the curve by the header's rule, as oracle_lib's native points."""
    out = []
    if curve == "g1":
        x = 2
        while len(out) < CANDIDATES:
            rhs = (x ** 3 + 3) % P
            y = pow(rhs, (P + 1) // 4, P)
            if rhs and y * y % P == rhs:
                out.append((x, min(y, P - y)))
            x += 1
        return out
    n = pow(82, P - 2, P)
    b = (27 * n % P, -3 * n % P)                       # 3 / (9 + i)
    assert _f2mul(b, (9, 1)) == (3, 0)
    k = 0
    while len(out) < CANDIDATES:
        x = (k, 1)
        x3 = _f2mul(_f2mul(x, x), x)
        rhs = ((x3[0] + b[0]) % P, (x3[1] + b[1]) % P)
        y = _f2sqrt(rhs) if rhs != (0, 0) else None
        if y is not None:
            out.append((x, min(y, ((-y[0]) % P, (-y[1]) % P), key=lambda v: (v[1], v[0]))))
        k += 1
    return out


def on_curve(curve, pt):
    if curve == "g1":
        return (pt[1] ** 2 - pt[0] ** 3 - 3) % P == 0
    n = pow(82, P - 2, P)
    x3 = _f2mul(_f2mul(pt[0], pt[0]), pt[0])
    y2 = _f2mul(pt[1], pt[1])
    return ((y2[0] - x3[0] - 27 * n) % P, (y2[1] - x3[1] + 3 * n) % P) == (0, 0)


# ---------------------------------------------------------------- the model
def effective(curve, xs, es, masks):
    """The effective terms: (generator, 0) where the mask is set."""
    return ([GEN[curve] if m else x for x, m in zip(xs, masks)], [0 if m else e for e, m in zip(es, masks)])


def choose_segment(curve, xs, es):
    """(choice, insts, final) of one segment: the smallest candidate from which no offset and no final is the point at infinity
    and Python's walk of every instance is clean; (None, first bad instance of candidate 7, None) when all eight fail."""
    bad = None
    for j, h in enumerate(candidates(curve)):
        insts, final = CL.derive(curve, xs, es, h)
        bad = CL.walk_all(curve, insts)
        if bad is None and final is None:
            bad = (len(insts) - 1, -1)
        if bad is None:
            return j, insts, final
    return None, bad[0], None


def model(curve, xs, es, lengths, masks=None):
    """(xs_eff, es_eff, choice, starts, insts, finals, sums) in Python integers."""
    masks = masks or [0] * len(xs)
    ex, ee = effective(curve, xs, es, masks)
    add, neg, _ = T._ops(curve)
    choice, starts, insts, finals = [], [], [], []
    for h, n in zip(MB.heads(lengths), lengths):
        j, seg, fin = choose_segment(curve, ex[h:h + n], ee[h:h + n])
        assert j is not None, "the segment exhausts the candidates"
        choice.append(j)
        starts.append(candidates(curve)[j])
        insts += seg
        finals.append(fin)
    return ex, ee, choice, starts, insts, finals, MB.sums_of(curve, finals, starts)


def sum_of(curve, xs, es):
    """sum e_k x_k by Python's complete addition, no start anywhere: None is the point at infinity."""
    add, _, mul = T._ops(curve)
    acc = None
    for x, e in zip(xs, es):
        acc = add(acc, mul(x, e))
    return acc


def kill(curve, j, prefix_xs, prefix_es, sign=1):
    """The x that kills candidate j right behind the given terms of a segment when its exponent has bit 0 set: x = +-(H_j + S), S
    the sum of those terms, so that the offset of the instance is +-x at the table's first addition."""
    add, neg, _ = T._ops(curve)
    x = add(candidates(curve)[j], sum_of(curve, prefix_xs, prefix_es))
    assert x is not None
    return x if sign > 0 else neg(x)


def _rnd(curve, rng):
    return O.g1_random(rng) if curve == "g1" else O.g2_random(rng)


def _exp(rng):
    return int.from_bytes(rng.bytes(32), "little") % R


def _benign(curve, rng, n):
    return [_rnd(curve, rng) for _ in range(n)], [_exp(rng) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def host_cases(curve):
    """{name: (xs, es, lengths, masks, want_choice)} for num_io = 4 (segments straddle the unit boundaries):
      random     11 random terms in segments of 1, 2, 5, 3: every choice 0;
      traps      what the generator as default start refuses: G and -G with odd scalars, alone and as the head of a segment: 0;
      head       a head +-candidate 0 with an odd scalar between benign neighbours (choice 1, neighbours 0), and a segment whose
                 head kills candidate 0 and whose second instance kills candidate 1 (choice 2);
      middle     (Q, 3) then x = candidate 0 + 3 Q with an odd scalar: choice 1; the segment behind it has the same partial sum
                 3 Q and a benign second term: 0;
      masks      masked terms whose words are >= p or off the curve (the caller's words: masked_words), a masked head, an all-masked
                 segment, zero scalars, a repeated point and a point with its negative (a sum at infinity)."""
    rng = np.random.default_rng(41)
    add, neg, mul = T._ops(curve)
    g, h0 = GEN[curve], candidates(curve)[0]
    out = {}
    xs, es = _benign(curve, rng, 11)
    out["random"] = (xs, es, [1, 2, 5, 3], None, [0, 0, 0, 0])
    bx, be = _benign(curve, rng, 3)
    out["traps"] = ([g, neg(g), g, bx[0], bx[1], neg(g), bx[2]], [_exp(rng) | 1, _exp(rng) | 1, 5, be[0], be[1], 7, be[2]], [1, 1, 3, 2], None, [0, 0, 0, 0])
    bx, be = _benign(curve, rng, 6)
    e0, e1 = _exp(rng) | 1, _exp(rng) | 1
    xs = [bx[0], bx[1], h0, bx[2], bx[3], neg(h0), bx[4], h0, None, bx[5]]
    es = [be[0], be[1], e0, be[2], be[3], 9, be[4], e0, e1, be[5]]
    xs[8] = kill(curve, 1, [h0], [e0])
    out["head"] = (xs, es, [2, 2, 1, 2, 3], None, [0, 1, 0, 1, 2])
    bx, be = _benign(curve, rng, 2)
    xs = [bx[0], kill(curve, 0, [bx[0]], [3]), bx[0], bx[1]]
    out["middle"] = (xs, [3, _exp(rng) | 1, 3, be[1]], [2, 2], None, [1, 0])
    bx, be = _benign(curve, rng, 6)
    xs = [bx[0], bx[1], bx[2], bx[3], bx[4], bx[0], bx[0], bx[5], neg(bx[5]), bx[2]]
    es = [be[0], be[1], 0, be[3], be[4], 0, be[0], be[5], be[5], 0]
    masks = [0, 1, 0, 1, 1, 1, 0, 0, 0, 0]
    out["masks"] = (xs, es, [3, 1, 2, 1, 2, 1], masks, [0, 0, 0, 0, 0, 0])
    for name, (xs, es, lengths, masks, want) in out.items():
        assert sum(lengths) == len(xs) == len(es), name
        assert model(curve, xs, es, lengths, masks)[2] == want, name
    _, _, _, starts, _, finals, sums = model(curve, *out["masks"][:4])
    assert [s for s, v in enumerate(sums) if v is None] == [1, 2, 4, 5] and finals[2] == starts[2]   # all-masked, (0 x, masked), x - x, 0 x
    return out


def masked_words(curve, terms, masks):
    """The caller's words of a masked list: the masked rows are overwritten with coordinates >= p (odd masked rows) or with a
    point off the curve and a non-zero exponent (even ones); the library must not read them."""
    terms = terms.copy()
    for k, m in enumerate(masks or []):
        if m and k % 2:
            terms[k, :] = 0xFFFFFFFF
        elif m:
            terms[k, 0] ^= 1
            terms[k, -8:] = 0xFFFFFFFF
    return terms


@functools.lru_cache(maxsize=None)
def exhausted(curve):
    """(xs, es, lengths, bad_segment, bad_instance): a benign segment of 2, then the 8-term segment with e_g = 1 and x_g = H_g +
    S_{g-1}, which candidate j cannot pass at instance j at the latest, then a benign segment of 1.  Candidate 7 fails at the
    segment's last instance, global instance 9."""
    rng = np.random.default_rng(43)
    bx, be = _benign(curve, rng, 3)
    kx, ke = [], []
    for j in range(CANDIDATES):
        kx.append(kill(curve, j, kx, ke))
        ke.append(1)
    j, at, _ = choose_segment(curve, kx, ke)
    assert j is None and at == 7
    xs, es = bx[:2] + kx + bx[2:], be[:2] + ke + be[2:]
    own = T._ops(curve)[2](GEN[curve], 12345)               # a start of the caller's own takes the same terms
    insts, final = CL.derive(curve, kx, ke, own)
    assert CL.walk_all(curve, insts) is None and final is not None
    return xs, es, [2, 8, 1], 1, 9, own


def words(curve, xs, es, masks=None):
    """The caller's terms: placeholders for the masked ones, then masked_words."""
    ex, ee = effective(curve, xs, es, masks or [0] * len(xs))
    return masked_words(curve, CL.terms_words(curve, ex, ee), masks)


# ---------------------------------------------------------------- the GPU recipes: built from kills, no Python walk of the whole unit
@functools.lru_cache(maxsize=None)
def unit_recipe(curve):
    """One unit of 121 instances of a table of 128 (np.random.default_rng(47)); (terms, lengths, masks, want_choice):
      segment 0  length 1, benign                          0      segment 5  33 benign terms                           0
      segment 1  the trap: head G, odd scalar              0      segment 6  a middle kill of candidate 0 at its third    1
      segment 2  head kill of candidate 0                  1      segment 7  all masked (3 terms)                      0
      segment 3  40 terms, term 7 masked                   0      segment 8  head kills 0, second instance kills 1     2
      segment 4  length 1, -G with an odd scalar           0      segment 9  benign, 12 terms                          0
    The expected choices follow from the kills (each asserted on its own segment by choose_segment); the benign segments are
    random, so any candidate passes them."""
    rng = np.random.default_rng(47)
    add, neg, mul = T._ops(curve)
    g, h0 = GEN[curve], candidates(curve)[0]
    lengths = [1, 5, 4, 40, 1, 33, 6, 3, 16, 12]
    xs, es = _benign(curve, rng, sum(lengths))
    hs = MB.heads(lengths)
    masks = [0] * len(xs)
    xs[hs[1]], es[hs[1]] = g, es[hs[1]] | 1
    xs[hs[2]], es[hs[2]] = neg(h0), es[hs[2]] | 1
    masks[hs[3] + 7] = 1
    xs[hs[4]], es[hs[4]] = neg(g), es[hs[4]] | 1
    a = hs[6]
    es[a], es[a + 1] = 3, 5
    xs[a + 2], es[a + 2] = kill(curve, 0, xs[a:a + 2], es[a:a + 2], -1), es[a + 2] | 1
    for k in range(hs[7], hs[8]):
        masks[k] = 1
    b = hs[8]
    xs[b], es[b] = h0, 1
    xs[b + 1], es[b + 1] = kill(curve, 1, [h0], [1]), es[b + 1] | 1
    want = [0, 0, 1, 0, 0, 0, 1, 0, 2, 0]
    for s in (1, 2, 4, 6, 8):                                # the short segments with a kill: Python's walk agrees
        ex, ee = xs[hs[s]:hs[s] + lengths[s]], es[hs[s]:hs[s] + lengths[s]]
        assert choose_segment(curve, ex, ee)[0] == want[s], s
    assert sum(lengths) == 121
    return words(curve, xs, es, masks), MB.lengths_words(lengths), np.array(masks, dtype=np.uint8), want


@functools.lru_cache(maxsize=None)
def unit_exhausted(curve):
    """The exhausted list as caller's words: (terms, lengths)."""
    xs, es, lengths, _, _, _ = exhausted(curve)
    return CL.terms_words(curve, xs, es), MB.lengths_words(lengths)


@functools.lru_cache(maxsize=None)
def block_recipe():
    """G1, a table of 1,024 instances: the smallest whose unit the scan takes in blocks of 512 lanes (chain_scan: K > CS_LANES).
    700 terms in segments of 7; segment 10 (instances 70 .. 76, block 0) kills candidate 0 at its head, segment 90 (630 .. 636,
    block 1) kills candidates 0 and 1; segment 73 (511 .. 517) straddles the two blocks.  (terms, lengths, want_choice)."""
    rng = np.random.default_rng(53)
    h0 = candidates("g1")[0]
    lengths = [7] * 100
    xs, es = _benign("g1", rng, 700)
    xs[70], es[70] = h0, es[70] | 1
    xs[630], es[630] = h0, 1
    xs[631], es[631] = kill("g1", 1, [h0], [1]), es[631] | 1
    want = [0] * 100
    want[10], want[90] = 1, 2
    for s in (10, 90):
        assert choose_segment("g1", xs[7 * s:7 * s + 7], es[7 * s:7 * s + 7])[0] == want[s]
    return CL.terms_words("g1", xs, es), MB.lengths_words(lengths), want


@functools.lru_cache(maxsize=None)
def batch_recipe():
    """G1, 300 instances in 3 units of 128 (MB.BATCH_LENGTHS: a segment across each unit boundary): segment 3 takes a head kill
    of candidate 0, instance 200 is masked, segment 5 is the trap (head G, odd scalar).  (terms, lengths, masks, want_choice)."""
    num_io, lengths = MB.BATCH_LENGTHS["g1"]
    rng = np.random.default_rng(59)
    xs, es = _benign("g1", rng, sum(lengths))
    hs = MB.heads(lengths)
    masks = [0] * len(xs)
    xs[hs[3]], es[hs[3]] = candidates("g1")[0], es[hs[3]] | 1
    xs[hs[5]], es[hs[5]] = GEN["g1"], es[hs[5]] | 1
    masks[200] = 1
    want = [0] * len(lengths)
    want[3] = 1
    assert choose_segment("g1", xs[hs[3]:hs[3] + lengths[3]], es[hs[3]:hs[3] + lengths[3]])[0] == 1
    return words("g1", xs, es, masks), MB.lengths_words(lengths), np.array(masks, dtype=np.uint8), want
