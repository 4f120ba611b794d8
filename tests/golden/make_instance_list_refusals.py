"""Records what the host entry points of the five instance-list units answer, case by case, into instance_list_refusals.json:

    python tests/golden/make_instance_list_refusals.py          (SBN_LIB selects the library, as everywhere)

The units are csrc/chain_instances.hip, msm.hip, scalar_mul.hip, powers.hip and msm_batch.hip; the entry points are
sbn_chain_instances, sbn_msm_instances, sbn_msm_check_links, sbn_scalar_mul_instances, sbn_scalar_mul_check,
sbn_mul_by_cofactor_check, sbn_power_instances, sbn_power_check, sbn_msm_batch_instances, sbn_msm_batch_check,
sbn_curve_generator, sbn_g2_cofactor and sbn_bn_x.  A case names a builder of this file and its parameters (the inputs are derived
in Python integers through tests/chained_lists.py, scalar_mul_lists.py, power_lists.py and msm_batches.py (which cuts its lists
into units through msm_lists.py), never by the library), and records the return code, the full sbn_last_error() text and, for accepted calls, the SHA-256 of every output
array.  Before every call the error text is set to a known one (a refused sbn_g2_cofactor(NULL)), so an accepted call records that
it left the text alone.  tests/test_instance_list_refusals_host.py replays the file against the library under test.

The file was recorded with the library of the commit BEFORE the five units were folded onto one shared header, and every later
library has to answer the same bytes.  At that commit the five units held 91 `fail(` call sites.  Every one is hit by at least
one case here, except four that no call through the ABI reaches:
  * scalar_mul.hip "degenerate affine operation (x1 == x2 or y == 0)" behind name_degenerate, and its twin in msm_batch.hip behind
    first_bad: reached only when the table's walk of a chunk fails and the one-instance form of the SAME walk then finds no
    failing instance -- the two run the same code on the same rows;
  * msm_batch.hip "kind %d is not an Exp table" in msm_batch_check_inputs and in msm_batch_derive: every caller has passed
    msm_batch_check_args, which refuses such a kind first (with its own, longer text).
Shapes: num_io is a free argument of these host calls, so the lists hold 3 .. 7 instances in units of 2 .. 4; three lists of 520
curve instances (small exponents keep Python quick) carry a degenerate instance at 515, behind the 512-instance chunk of the
table's walk, each with its accepted twin."""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import chained_lists as CL  # noqa: E402
import msm_batches as MB  # noqa: E402
import oracle_lib as O  # noqa: E402
import power_lists as PL  # noqa: E402
import scalar_mul_lists as SM  # noqa: E402
import tracegen_edges as T  # noqa: E402

OUT = os.path.join(HERE, "instance_list_refusals.json")
P, R, GLP = T.P, T.R, T.GLP
NAMED = {"P": P, "GLP": GLP}
TABLES = ["g1", "g2", "fq", "fq12", "fq12u64"]
CURVES, FIELDS = TABLES[:2], TABLES[2:]
# u32 words of a value and of the exponent in `ios`; public inputs per value and per exponent; bits of a public-input limb
GEOM = {"g1": (16, 8, 16, 8, 32), "g2": (32, 8, 32, 8, 32), "fq": (8, 8, 8, 8, 32), "fq12": (96, 8, 192, 8, 16), "fq12u64": (96, 2, 192, 1, 16)}


def per_instance(table):
    _, _, W, EW, _ = GEOM[table]
    return 3 * W + EW


def pi_at(table, num_io, g, field, limb=0):
    """[unit, column] of a limb of instance g in the public inputs of the units."""
    _, _, W, EW, _ = GEOM[table]
    return [g // num_io, per_instance(table) * (g % num_io) + {"x": 0, "offset": W, "exponent": 2 * W, "output": 2 * W + EW}[field] + limb]


# ---------------------------------------------------------------- Python values -> words
def value_pi(table, v):
    bits = GEOM[table][4]
    return [l for c in CL._flat(table, v) for l in T.limbs(c, 256 // bits, bits)]


def exp_pi(table, e):
    return [e] if table == "fq12u64" else T.limbs(e, 8, 32)


def pi_units(table, insts, outs, num_io):
    rows = [value_pi(table, x) + value_pi(table, off) + exp_pi(table, e) + value_pi(table, out) for (x, off, e), out in zip(insts, outs)]
    while len(rows) % num_io:
        rows.append(rows[-1])
    return np.array(rows, dtype=np.uint64).reshape(len(rows) // num_io, -1)


def _rand_value(table, rng):
    if table in CURVES:
        return (O.g1_random if table == "g1" else O.g2_random)(rng)
    rand = lambda: int.from_bytes(rng.bytes(32), "little") % P   # noqa: E731
    return rand() if table == "fq" else [rand() for _ in range(12)]


def _rand_exp(table, rng, small):
    if small:
        return int(rng.integers(2, 256))
    e = int.from_bytes(rng.bytes(32), "little")
    return e % GLP if table == "fq12u64" else (e % R if table in CURVES else e)


# ---------------------------------------------------------------- the lists, in Python integers
@functools.lru_cache(maxsize=None)
def _segmented_base(table, lengths, seed, small, starts):
    """(xs, es, start values per segment, insts, finals): M = sum(lengths) instances, exponent 0 at instance 1.
    starts: 'per' (curves: (s + 2) * generator; fields: random), 'shared' (twice the generator; random) or 'default' (the generator;
    one)."""
    rng = np.random.default_rng(seed)
    M = sum(lengths)
    xs = [_rand_value(table, rng) for _ in range(M)]
    es = [_rand_exp(table, rng, small) for _ in range(M)]
    es[1] = 0
    if table in CURVES:
        _, neg, mul = T._ops(table)
        gen = CL.START[table]
        sv = {"per": [mul(gen, s + 2) for s in range(len(lengths))], "shared": [mul(gen, 2)] * len(lengths), "default": [gen] * len(lengths)}[starts]
    else:
        one = 1 if table == "fq" else list(CL.ONE12)
        shared = _rand_value(table, rng)
        sv = {"per": [_rand_value(table, rng) for _ in lengths], "shared": [shared] * len(lengths), "default": [one] * len(lengths)}[starts]
    insts, finals = MB.derive(table, xs, es, lengths, sv)
    return xs, es, sv, insts, finals


@functools.lru_cache(maxsize=None)
def _segmented_py(table, lengths, seed, small, starts, variant, at):
    """(xs, es, start values per segment, insts, outs) of that list, changed at instance `at` (curves): 'infinity' x = -offset, e = 1;
    'collide' x = offset and an odd e; 'twin' the same, e even.  Only the rest of that instance's segment is derived again."""
    xs, es, sv, insts, finals = (list(v) for v in _segmented_base(table, lengths, seed, small, starts))
    M = len(xs)
    if variant:
        s, h = max((s, h) for s, h in enumerate(MB.heads(lengths)) if h <= at)
        off, end = insts[at][1], h + lengths[s]
        xs[at] = T._ops(table)[1](off) if variant == "infinity" else off
        es[at] = 1 if variant == "infinity" else ((es[at] | 1) if variant == "collide" else (es[at] | 1) + 1)
        insts[at:end], finals[s] = CL.derive(table, xs[at:end], es[at:end], off)
    tails = {h + n - 1: s for s, (h, n) in enumerate(zip(MB.heads(lengths), lengths))}
    outs = [finals[tails[g]] if g in tails else insts[g + 1][1] for g in range(M)]
    return xs, es, sv, insts, outs


def _alloc(d, **shapes):
    d["_alloc"] = shapes
    return d


def segmented(table, lengths, seed, num_io, small=False, starts="per", variant=None, at=None, pi=False):
    """The arguments of the chained calls (one segment) and of the segmented ones."""
    xs, es, sv, insts, outs = _segmented_py(table, tuple(lengths), seed, small, starts, variant, at)
    xw, ew = GEOM[table][:2]
    M, S = len(xs), len(lengths)
    sw = MB.starts_words(table, sv if starts == "per" else sv[:1])
    d = {"kind": T.AIR[table], "terms": CL.terms_words(table, xs, es), "count": M, "start": sw[0].copy(), "lengths": MB.lengths_words(lengths), "segments": S,
         "starts": None if starts == "default" else sw, "start_count": S if starts == "per" else 1, "num_io": num_io, "curve": table in CURVES}
    if pi:
        d["pi"] = pi_units(table, insts, outs, num_io)
    units = -(-M // num_io)
    return _alloc(d, ios=(units * num_io, 2 * xw + ew), final=(xw,), finals=(S, xw), sums=(S, xw), infinity=(S,))


@functools.lru_cache(maxsize=None)
def _scalar_py(curve, count, seed, small, shared, offset, cofactor, variant, at, outputs):
    rng = np.random.default_rng(seed)
    add, neg, mul = T._ops(curve)
    off = mul(SM.GEN[curve], 2) if offset == "double" else SM.GEN[curve]
    xs = [_rand_value(curve, rng) for _ in range(count)]
    es = [_rand_exp(curve, rng, small) for _ in range(count)]
    es[1] = 0
    if shared:
        es = [SM.G2_COFACTOR if cofactor else es[0]] * count
    if variant:
        xs[at], es[at] = off, (es[at] | 1) if variant == "collide" else (es[at] | 1) + 1
    return xs, es, off, [add(off, mul(x, e)) for x, e in zip(xs, es)] if outputs else None


def scalar(curve, count, seed, num_io, small=False, shared=False, offset="gen", cofactor=False, variant=None, at=None, pi=False):
    """Independent scalar multiplications: exponent 0 at instance 1 (its product is the point at infinity); offset 'gen' (passed),
    'default' (NULL) or 'double' (twice the generator); shared: one scalar for all; cofactor: that scalar is 2p - r."""
    xs, es, off, outs = _scalar_py(curve, count, seed, small, shared, offset, cofactor, variant, at, pi)
    w = GEOM[curve][0]
    d = {"kind": T.AIR[curve], "points": SM.point_words(curve, xs), "scalars": SM.scalar_words(es[:1] if shared else es), "scalar_count": 1 if shared else count,
         "count": count, "num_io": num_io, "offset": None if offset == "default" else CL.value_words(curve, off)}
    if pi:
        d["pi"] = pi_units(curve, SM.explicit(curve, xs, es, off), outs, num_io)
    units = -(-count // num_io)
    return _alloc(d, ios=(units * num_io, 2 * w + 8), products=(count, w), infinity=(count,))


@functools.lru_cache(maxsize=None)
def _powers_py(table, count, depth, seed, shared, outputs):
    rng = PL.rng(seed)
    bases = [PL.random_elem(table, rng) for _ in range(count)]
    exps = [rng.randrange(GLP if table == "fq12u64" else 1 << 256) for _ in range(1 if shared else count)]
    if count > 1:
        bases[1] = 0 if table == "fq" else [0] * 12
    if not shared and count > 2:
        exps[2] = 0
    return bases, exps, PL.towers(table, bases, exps, depth) if outputs else None


def powers(table, count, depth, seed, num_io, shared=False, pi=False):
    """`count` towers of `depth` levels: base zero in tower 1, exponent 0 in tower 2 (per-tower exponents)."""
    w, ew = PL.WORDS[table]
    bases, exps, pw = _powers_py(table, count, depth, seed, shared, pi)
    d = {"kind": T.AIR[table], "bases": PL.base_words(table, bases), "exps": PL.exp_words(table, exps), "exp_count": len(exps), "count": count, "depth": depth,
         "num_io": num_io}
    M = count * depth
    if pi:
        one = 1 if table == "fq" else list(CL.ONE12)
        insts = [(bases[k] if l == 0 else pw[k][l - 1], one, exps[0] if shared else exps[k]) for k in range(count) for l in range(depth)]
        d["pi"] = pi_units(table, insts, [v for lv in pw for v in lv], num_io)
    return _alloc(d, ios=(-(-M // num_io) * num_io, 2 * w + ew), powers=(M, w))


def constant(table=None):
    return _alloc({"kind": T.AIR[table] if table else 0}, out=(32,))


BUILDERS = {"segmented": segmented, "scalar": scalar, "powers": powers, "constant": constant}


# ---------------------------------------------------------------- one call
def _ptr(a):
    return None if a is None else a.ctypes.data


def _units(d):
    """The `public_inputs` argument: one pointer per unit (a unit listed in null_units: NULL)."""
    if d.get("pi") is None:
        return None
    rows = d["pi"]
    return (C.c_void_p * max(len(rows), 1))(*[None if u in d.get("null_units", ()) else rows[u].ctypes.data for u in range(len(rows))])


def _call(L, entry, d):
    """(rc, {name: output array})."""
    o = {k: np.zeros(shape, dtype=np.uint8 if k == "infinity" else np.uint32) for k, shape in d["_alloc"].items() if k not in d.get("without", ())}
    g = lambda k: _ptr(o.get(k))   # noqa: E731
    n_units = d.get("units", len(d["pi"]) if d.get("pi") is not None else 0)
    if entry == "sbn_chain_instances":
        rc = L.sbn_chain_instances(d["kind"], _ptr(d["terms"]), d["count"], _ptr(d["start"]), g("ios"), g("final"))
        keep = ("ios", "final")
    elif entry == "sbn_msm_instances":
        rc = L.sbn_msm_instances(d["kind"], _ptr(d["terms"]), d["count"], d["num_io"], _ptr(d["start"]), g("ios"), g("final"))
        keep = ("ios", "final")
    elif entry == "sbn_msm_check_links":
        rc = L.sbn_msm_check_links(d["kind"], d["num_io"], _units(d), n_units, d["count"], _ptr(d["terms"]) if d.get("with_terms") else None, _ptr(d["start"]), g("final"))
        keep = ("final",)
    elif entry == "sbn_scalar_mul_instances":
        rc = L.sbn_scalar_mul_instances(d["kind"], _ptr(d["points"]), _ptr(d["scalars"]), d["scalar_count"], d["count"], d["num_io"], _ptr(d["offset"]), g("ios"),
                                        g("products"), g("infinity"))
        keep = ("ios", "products", "infinity")
    elif entry == "sbn_scalar_mul_check":
        rc = L.sbn_scalar_mul_check(d["kind"], d["num_io"], _units(d), n_units, d["count"], _ptr(d["points"]), _ptr(d["scalars"]), d["scalar_count"], _ptr(d["offset"]),
                                    g("products"), g("infinity"))
        keep = ("products", "infinity")
    elif entry == "sbn_mul_by_cofactor_check":
        rc = L.sbn_mul_by_cofactor_check(d["num_io"], _units(d), n_units, d["count"], _ptr(d["points"]), g("products"), g("infinity"))
        keep = ("products", "infinity")
    elif entry == "sbn_power_instances":
        rc = L.sbn_power_instances(d["kind"], _ptr(d["bases"]), _ptr(d["exps"]), d["exp_count"], d["count"], d["depth"], d["num_io"], g("ios"), g("powers"))
        keep = ("ios", "powers")
    elif entry == "sbn_power_check":
        rc = L.sbn_power_check(d["kind"], d["num_io"], _units(d), n_units, d["count"], d["depth"], _ptr(d["bases"]), _ptr(d["exps"]), d["exp_count"], g("powers"))
        keep = ("powers",)
    elif entry in ("sbn_msm_batch_instances", "sbn_msm_batch_check"):
        curve_outs = d["curve"] or d.get("force_sums")
        sums, inf = (g("sums"), g("infinity")) if curve_outs else (None, None)
        if entry == "sbn_msm_batch_instances":
            rc = L.sbn_msm_batch_instances(d["kind"], _ptr(d["terms"]), _ptr(d["lengths"]), d["segments"], _ptr(d["starts"]), d["start_count"], d["num_io"], g("ios"),
                                           g("finals"), sums, inf)
        else:
            rc = L.sbn_msm_batch_check(d["kind"], d["num_io"], _units(d), n_units, _ptr(d["lengths"]), d["segments"], _ptr(d["terms"]) if d.get("with_terms") else None,
                                       _ptr(d["starts"]), d["start_count"], g("finals"), sums, inf)
        keep = (("ios",) if entry == "sbn_msm_batch_instances" else ()) + ("finals",) + (("sums", "infinity") if curve_outs else ())
    elif entry == "sbn_curve_generator":
        rc = L.sbn_curve_generator(d["kind"], g("out"))
        keep = ("out",)
    elif entry == "sbn_g2_cofactor":
        rc = L.sbn_g2_cofactor(g("out"))
        keep = ("out",)
    elif entry == "sbn_bn_x":
        rc = L.sbn_bn_x(g("out"))
        keep = ("out",)
    else:
        raise KeyError(entry)
    return rc, {k: o[k] for k in keep if k in o}


def run_case(L, case):
    """(rc, sbn_last_error() text, {output: sha256} or None) of one recorded case on the library L (ctypes, argtypes set)."""
    prm = dict(case["params"])
    edits, null, args = prm.pop("edits", ()), prm.pop("null", ()), prm.pop("args", {})
    how = {k: prm.pop(k) for k in ("without", "with_terms", "null_units", "force_sums") if k in prm}   # how the call is made, not what the list is
    d = BUILDERS[case["builder"]](**prm)
    d.update(how)
    for name, index, op, value in edits:      # after the builder: what the caller hands in is no longer the list Python derived
        a, value = d[name], NAMED.get(value, value) if isinstance(value, str) else value
        if op == "limbs":                     # eight u32 limbs of `value` from the index on
            row = a[tuple(index[:-1])]
            row[index[-1]:index[-1] + 8] = T.limbs(value, 8, 32)
        else:
            a[tuple(index)] = (int(a[tuple(index)]) ^ value) if op == "xor" else value
    d.update(args)
    for name in null:
        d[name] = None
    assert L.sbn_g2_cofactor(None) == -1    # a known error text: an accepted call leaves it as it is
    rc, outs = _call(L, case["call"], d)
    text = L.sbn_last_error().decode()
    return rc, text, ({k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in outs.items()} if rc == 0 else None)


# ---------------------------------------------------------------- the cases
def _cases():
    cases = []

    def add(call, builder, want, edits=(), null=(), args=None, **params):
        if edits:
            params["edits"] = [list(e) for e in edits]
        if null:
            params["null"] = list(null)
        if args:
            params["args"] = args
        cases.append(({"call": call, "builder": builder, "params": params}, want))

    OK, BAD_ARG, NON_CANONICAL, VERIFY, UNSUPPORTED, WITNESS = 0, -1, -2, -6, -7, -8
    seg = lambda t, n=5, **kw: dict(table=t, lengths=[n], seed=41, num_io=2, **kw)   # noqa: E731
    xw = lambda t: GEOM[t][0]   # noqa: E731

    # ---- chained lists: sbn_chain_instances, and the same lists cut into units by sbn_msm_instances
    for call in ("sbn_chain_instances", "sbn_msm_instances"):
        for t in TABLES:
            add(call, "segmented", OK, **seg(t, starts="shared"))
            add(call, "segmented", BAD_ARG, edits=[("terms", [2, xw(t) - 8], "limbs", "P")], **seg(t, starts="shared"))                 # >= p, an instance
            add(call, "segmented", BAD_ARG, edits=[("start", [xw(t) - 8], "limbs", "P")], **seg(t, starts="shared"))            # >= p, the start
        add(call, "segmented", OK, without=["final"], **seg("g1", starts="shared"))
        add(call, "segmented", NON_CANONICAL, edits=[("terms", [3, 96], "set", 1), ("terms", [3, 97], "set", 0xFFFFFFFF)], **seg("fq12u64", starts="shared"))
        add(call, "segmented", BAD_ARG, null=["terms"], **seg("g1"))
        add(call, "segmented", BAD_ARG, null=["start"], **seg("fq"))
        add(call, "segmented", BAD_ARG, without=["ios"], **seg("fq12"))
        add(call, "segmented", BAD_ARG, args={"count": 0}, **seg("g2"))
        add(call, "segmented", BAD_ARG, args={"kind": 1}, **seg("g1"))
        add(call, "segmented", BAD_ARG, args={"kind": 99}, **seg("fq"))
        for t in CURVES:
            add(call, "segmented", BAD_ARG, edits=[("terms", [3, 0], "xor", 1), ("terms", [4, 0], "xor", 1)], **seg(t))         # off the curve: the first one is named
            add(call, "segmented", BAD_ARG, edits=[("start", [0], "xor", 1)], **seg(t))
            add(call, "segmented", WITNESS, **seg(t, variant="infinity", at=0))
            add(call, "segmented", WITNESS, **seg(t, variant="infinity", at=2))
            add(call, "segmented", WITNESS, **seg(t, variant="infinity", at=4))                                                  # the last output
            add(call, "segmented", WITNESS, **seg(t, variant="collide", at=3))
            add(call, "segmented", OK, **seg(t, variant="twin", at=3))
    add("sbn_msm_instances", "segmented", BAD_ARG, args={"num_io": 0}, **seg("g1"))
    add("sbn_msm_instances", "segmented", OK, table="fq", lengths=[4], seed=41, num_io=4)                                        # no pad row
    add("sbn_msm_instances", "segmented", OK, table="fq12", lengths=[3], seed=41, num_io=8)                                      # one unit, five pads
    # more than 512 instances on G1: the walk crosses its chunk boundary, the degenerate instance sits in the second chunk
    long_ = dict(table="g1", lengths=[520], seed=43, num_io=64, small=True)
    add("sbn_msm_instances", "segmented", OK, **long_)
    add("sbn_msm_instances", "segmented", WITNESS, variant="collide", at=515, **long_)
    add("sbn_msm_instances", "segmented", OK, variant="twin", at=515, **long_)
    add("sbn_msm_instances", "segmented", WITNESS, variant="infinity", at=515, **long_)

    # ---- sbn_msm_check_links
    for t in TABLES:
        c = seg(t, starts="shared", pi=True)   # 5 instances in units of 2: three units, one pad
        add("sbn_msm_check_links", "segmented", OK, **c)
        add("sbn_msm_check_links", "segmented", OK, with_terms=True, **c)
        add("sbn_msm_check_links", "segmented", VERIFY, edits=[("start", [1], "xor", 1)], **c)
        add("sbn_msm_check_links", "segmented", VERIFY, with_terms=True, edits=[("terms", [3, 2], "xor", 1 << 16)], **c)
        add("sbn_msm_check_links", "segmented", VERIFY, with_terms=True, edits=[("terms", [4, xw(t)], "xor", 1)], **c)
        add("sbn_msm_check_links", "segmented", VERIFY, edits=[("pi", pi_at(t, 2, 1, "output", 3), "xor", 1)], **c)               # the link across the unit boundary
        add("sbn_msm_check_links", "segmented", VERIFY, edits=[("pi", pi_at(t, 2, 4, "output", 1), "set", 1 << 32), ("pi", pi_at(t, 2, 5, "output", 1), "set", 1 << 32)], **c)
        add("sbn_msm_check_links", "segmented", VERIFY if GEOM[t][4] == 16 else OK,      # wider than a 16-bit limb only
            edits=[("pi", pi_at(t, 2, 4, "output", 1), "set", 1 << 16), ("pi", pi_at(t, 2, 5, "output", 1), "set", 1 << 16)], **c)
    c = seg("g2", starts="shared", pi=True)
    for f in ("x", "offset", "exponent", "output"):
        add("sbn_msm_check_links", "segmented", VERIFY, edits=[("pi", pi_at("g2", 2, 5, f, 2), "xor", 1)], **c)
        add("sbn_msm_check_links", "segmented", VERIFY, edits=[("pi", pi_at("fq12u64", 2, 5, f, 0), "xor", 1)], **seg("fq12u64", starts="shared", pi=True))
    add("sbn_msm_check_links", "segmented", BAD_ARG, args={"kind": 7}, **c)
    add("sbn_msm_check_links", "segmented", BAD_ARG, null=["pi"], args={"units": 3}, **c)
    add("sbn_msm_check_links", "segmented", BAD_ARG, null=["start"], **c)
    add("sbn_msm_check_links", "segmented", BAD_ARG, args={"count": 0}, **c)
    add("sbn_msm_check_links", "segmented", BAD_ARG, args={"num_io": 0}, **c)
    add("sbn_msm_check_links", "segmented", VERIFY, args={"units": 2}, **c)
    add("sbn_msm_check_links", "segmented", VERIFY, args={"count": 7}, **c)
    add("sbn_msm_check_links", "segmented", BAD_ARG, null_units=[1], **c)
    add("sbn_msm_check_links", "segmented", OK, without=["final"], **c)

    # ---- independent scalar multiplications
    sc = lambda t, **kw: dict(curve=t, count=5, seed=47, num_io=2, **kw)   # noqa: E731
    for t in CURVES:
        add("sbn_scalar_mul_instances", "scalar", OK, **sc(t))
        add("sbn_scalar_mul_instances", "scalar", OK, **sc(t, shared=True, offset="default"))
        add("sbn_scalar_mul_instances", "scalar", OK, without=["ios"], **sc(t, offset="double"))
        add("sbn_scalar_mul_instances", "scalar", OK, without=["products", "infinity"], **sc(t))
        add("sbn_scalar_mul_instances", "scalar", BAD_ARG, edits=[("points", [2, 8], "limbs", "P")], **sc(t))
        add("sbn_scalar_mul_instances", "scalar", BAD_ARG, edits=[("offset", [0], "limbs", "P")], **sc(t))
        add("sbn_scalar_mul_instances", "scalar", BAD_ARG, edits=[("offset", [0], "xor", 1)], **sc(t))
        add("sbn_scalar_mul_instances", "scalar", BAD_ARG, edits=[("points", [3, 0], "xor", 1), ("points", [1, 0], "xor", 1)], **sc(t))
        add("sbn_scalar_mul_instances", "scalar", WITNESS, **sc(t, variant="collide", at=3))
        add("sbn_scalar_mul_instances", "scalar", WITNESS, **sc(t, variant="collide", at=3, offset="default"))
        add("sbn_scalar_mul_instances", "scalar", OK, **sc(t, variant="twin", at=3))
    add("sbn_scalar_mul_instances", "scalar", UNSUPPORTED, args={"kind": T.AIR["fq"]}, **sc("g1"))
    add("sbn_scalar_mul_instances", "scalar", BAD_ARG, null=["points"], **sc("g1"))
    add("sbn_scalar_mul_instances", "scalar", BAD_ARG, null=["scalars"], **sc("g2"))
    add("sbn_scalar_mul_instances", "scalar", BAD_ARG, args={"count": 0}, **sc("g1"))
    add("sbn_scalar_mul_instances", "scalar", BAD_ARG, args={"num_io": 0}, **sc("g1"))
    add("sbn_scalar_mul_instances", "scalar", BAD_ARG, args={"scalar_count": 2}, **sc("g1"))
    long_sc = dict(curve="g1", count=520, seed=53, num_io=64, small=True)
    add("sbn_scalar_mul_instances", "scalar", OK, **long_sc)
    add("sbn_scalar_mul_instances", "scalar", WITNESS, variant="collide", at=515, **long_sc)
    add("sbn_scalar_mul_instances", "scalar", OK, variant="twin", at=515, **long_sc)
    for t in CURVES:
        c = sc(t, pi=True)
        add("sbn_scalar_mul_check", "scalar", OK, **c)
        add("sbn_scalar_mul_check", "scalar", OK, **sc(t, pi=True, shared=True, offset="default"))
        add("sbn_scalar_mul_check", "scalar", OK, without=["products", "infinity"], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("points", [2, 1], "xor", 1)], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("scalars", [4, 7], "xor", 1)], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("pi", pi_at(t, 2, 3, "offset", 0), "xor", 1)], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("pi", pi_at(t, 2, 2, "output", 5), "set", 1 << 32)], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("pi", pi_at(t, 2, 2, "output", i), "set", l) for i, l in enumerate(T.limbs(P, 8, 32))], **c)
        add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("pi", pi_at(t, 2, 0, "output", 0), "xor", 1)], **c)
        add("sbn_scalar_mul_check", "scalar", BAD_ARG, edits=[("offset", [8], "limbs", "P")], **c)
        for f in ("x", "offset", "exponent", "output"):
            add("sbn_scalar_mul_check", "scalar", VERIFY, edits=[("pi", pi_at(t, 2, 5, f, 1), "xor", 1)], **c)
    c = sc("g1", pi=True)
    add("sbn_scalar_mul_check", "scalar", UNSUPPORTED, args={"kind": T.AIR["fq12"]}, **c)
    add("sbn_scalar_mul_check", "scalar", BAD_ARG, null=["pi"], args={"units": 3}, **c)
    add("sbn_scalar_mul_check", "scalar", BAD_ARG, null=["points"], **c)
    add("sbn_scalar_mul_check", "scalar", BAD_ARG, args={"scalar_count": 3}, **c)
    add("sbn_scalar_mul_check", "scalar", VERIFY, args={"units": 4}, **c)
    add("sbn_scalar_mul_check", "scalar", BAD_ARG, null_units=[0, 2], **c)
    cf = dict(curve="g2", count=3, seed=59, num_io=2, shared=True, cofactor=True, pi=True)
    add("sbn_mul_by_cofactor_check", "scalar", OK, **cf)
    add("sbn_mul_by_cofactor_check", "scalar", OK, without=["products", "infinity"], **cf)
    add("sbn_mul_by_cofactor_check", "scalar", VERIFY, **sc("g2", pi=True, shared=True))                                          # another scalar than 2p - r
    add("sbn_mul_by_cofactor_check", "scalar", VERIFY, **dict(cf, offset="double"))                                               # another offset than the generator
    add("sbn_mul_by_cofactor_check", "scalar", BAD_ARG, null=["pi"], args={"units": 2}, **cf)
    add("sbn_mul_by_cofactor_check", "scalar", BAD_ARG, null=["points"], **cf)
    add("sbn_mul_by_cofactor_check", "scalar", VERIFY, args={"units": 1}, **cf)
    add("sbn_mul_by_cofactor_check", "scalar", VERIFY, edits=[("pi", pi_at("g2", 2, 3, "x", 0), "xor", 1)], **cf)

    # ---- field powers and towers
    # three towers of three levels in units of four: M = 9, towers 1 and 2 straddle a unit boundary, rows 9 .. 11 are pads
    pw = lambda t, **kw: dict(table=t, count=3, depth=3, seed=61, num_io=4, **kw)   # noqa: E731
    for t in FIELDS:
        ew = GEOM[t][1]
        add("sbn_power_instances", "powers", OK, **pw(t))
        add("sbn_power_instances", "powers", OK, **pw(t, shared=True))
        add("sbn_power_instances", "powers", OK, without=["ios"], **pw(t))
        add("sbn_power_instances", "powers", OK, without=["powers"], **pw(t))
        add("sbn_power_instances", "powers", OK, table=t, count=2, depth=1, seed=61, num_io=2)                                   # independent powers, no pad
        add("sbn_power_instances", "powers", BAD_ARG, edits=[("bases", [2, xw(t) - 8], "limbs", "P")], **pw(t))
        add("sbn_power_check", "powers", OK, **pw(t, pi=True))
        add("sbn_power_check", "powers", OK, without=["powers"], **pw(t, pi=True, shared=True))
        c = pw(t, pi=True)
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 3, "offset", 0), "xor", 3)], **c)
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 2, "offset", 5), "set", 1)], **c)
        add("sbn_power_check", "powers", VERIFY, edits=[("exps", [1, ew - 1], "xor", 1)], **c)
        add("sbn_power_check", "powers", VERIFY, edits=[("bases", [2, 3], "xor", 1)], **c)
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 3, "output", 2), "xor", 1)], **c)                      # level 1 of tower 1 reads it across the unit boundary
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 2, "x", 2), "xor", 1)], **c)
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 2, "output", 2), "set", 1 << 32)], **c)
        add("sbn_power_check", "powers", VERIFY if GEOM[t][4] == 16 else OK, edits=[("pi", pi_at(t, 4, 2, "output", 2), "set", 1 << 16)], **c)   # wider than a 16-bit limb only
        n = 256 // GEOM[t][4]
        add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 1, "output", i), "set", l) for i, l in enumerate(T.limbs(P, n, GEOM[t][4]))], **c)
        for f in ("x", "offset", "exponent", "output"):
            add("sbn_power_check", "powers", VERIFY, edits=[("pi", pi_at(t, 4, 10, f, 0), "xor", 1)], **c)
    add("sbn_power_instances", "powers", NON_CANONICAL, edits=[("exps", [1, 0], "set", 1), ("exps", [1, 1], "set", 0xFFFFFFFF)], **pw("fq12u64"))
    add("sbn_power_instances", "powers", NON_CANONICAL, edits=[("exps", [0, 0], "set", 1), ("exps", [0, 1], "set", 0xFFFFFFFF)], **pw("fq12u64", shared=True))
    for call in ("sbn_power_instances", "sbn_power_check"):
        c = pw("fq", pi=call == "sbn_power_check")
        add(call, "powers", UNSUPPORTED, args={"kind": T.AIR["g1"]}, **c)
        add(call, "powers", UNSUPPORTED, args={"kind": 1}, **c)
        add(call, "powers", BAD_ARG, null=["bases"], **c)
        add(call, "powers", BAD_ARG, null=["exps"], **c)
        add(call, "powers", BAD_ARG, args={"count": 0}, **c)
        add(call, "powers", BAD_ARG, args={"depth": 0}, **c)
        add(call, "powers", BAD_ARG, args={"num_io": 0}, **c)
        add(call, "powers", BAD_ARG, args={"exp_count": 2}, **c)
        add(call, "powers", BAD_ARG, args={"depth": 1 << 63}, **c)
    c = pw("fq12", pi=True)
    add("sbn_power_check", "powers", BAD_ARG, null=["pi"], args={"units": 3}, **c)
    add("sbn_power_check", "powers", VERIFY, args={"units": 2}, **c)
    add("sbn_power_check", "powers", BAD_ARG, null_units=[1], **c)

    # ---- segmented lists
    sg = lambda t, **kw: dict(table=t, lengths=[1, 3, 2, 1], seed=67, num_io=4, **kw)   # noqa: E731   (heads 0 1 4 6; M = 7: one pad)
    for t in TABLES:
        for starts in ("per", "shared", "default"):
            add("sbn_msm_batch_instances", "segmented", OK, **sg(t, starts=starts))
            add("sbn_msm_batch_check", "segmented", OK, **sg(t, starts=starts, pi=True))
        add("sbn_msm_batch_instances", "segmented", OK, without=["ios"], **sg(t))
        add("sbn_msm_batch_instances", "segmented", OK, without=["finals", "sums", "infinity"], **sg(t))
        add("sbn_msm_batch_instances", "segmented", BAD_ARG, edits=[("terms", [5, xw(t) - 8], "limbs", "P")], **sg(t))
        add("sbn_msm_batch_instances", "segmented", BAD_ARG, edits=[("starts", [2, xw(t) - 8], "limbs", "P")], **sg(t))
        c = sg(t, pi=True)
        add("sbn_msm_batch_check", "segmented", OK, with_terms=True, **c)
        add("sbn_msm_batch_check", "segmented", OK, without=["finals", "sums", "infinity"], **c)
        add("sbn_msm_batch_check", "segmented", BAD_ARG, edits=[("starts", [3, 0], "limbs", "P")], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, with_terms=True, edits=[("terms", [5, 1], "xor", 1 << 16)], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, with_terms=True, edits=[("terms", [2, xw(t)], "xor", 1)], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("starts", [2, 0], "xor", 1)], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 4, "offset", 1), "xor", 1)], **c)               # a head, first of unit 1
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 2, "offset", 1), "xor", 1)], **c)               # a link
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 4, "output", 3), "set", 1 << 32)], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 4, "output", 3), "set", 1 << 16)], **c)
        for f in ("x", "offset", "exponent", "output"):
            add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 7, f, 0), "xor", 1)], **c)
    add("sbn_msm_batch_instances", "segmented", NON_CANONICAL, edits=[("terms", [4, 96], "set", 1), ("terms", [4, 97], "set", 0xFFFFFFFF)], **sg("fq12u64"))
    for t in CURVES:
        add("sbn_msm_batch_instances", "segmented", BAD_ARG, edits=[("terms", [5, 0], "xor", 1), ("terms", [2, 0], "xor", 1)], **sg(t))
        add("sbn_msm_batch_instances", "segmented", BAD_ARG, edits=[("starts", [1, 0], "xor", 1)], **sg(t))
        add("sbn_msm_batch_instances", "segmented", WITNESS, **sg(t, variant="infinity", at=2))                                   # the offset of instance 3
        add("sbn_msm_batch_instances", "segmented", WITNESS, **sg(t, variant="infinity", at=3))                                   # the output of a tail
        add("sbn_msm_batch_instances", "segmented", WITNESS, **sg(t, variant="infinity", at=0))                                   # a segment of one
        add("sbn_msm_batch_instances", "segmented", WITNESS, **sg(t, variant="collide", at=4))
        add("sbn_msm_batch_instances", "segmented", WITNESS, **sg(t, variant="collide", at=4, starts="default"))
        add("sbn_msm_batch_instances", "segmented", OK, **sg(t, variant="twin", at=4))
        c = sg(t, pi=True)
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 3, "output", i), "set", l) for i, l in enumerate(T.limbs(P, 8, 32))], **c)
        add("sbn_msm_batch_check", "segmented", VERIFY, edits=[("pi", pi_at(t, 4, 3, "output", 0), "xor", 1)], **c)              # a tail: no link reads it
        add("sbn_msm_batch_check", "segmented", OK, **sg(t, pi=True, variant="twin", at=4))
    long_sg = dict(table="g1", lengths=[4] * 130, seed=71, num_io=64, small=True)
    add("sbn_msm_batch_instances", "segmented", OK, **long_sg)
    add("sbn_msm_batch_instances", "segmented", WITNESS, variant="collide", at=515, **long_sg)
    add("sbn_msm_batch_instances", "segmented", OK, variant="twin", at=515, **long_sg)
    add("sbn_msm_batch_instances", "segmented", WITNESS, variant="infinity", at=517, **long_sg)
    for call in ("sbn_msm_batch_instances", "sbn_msm_batch_check"):
        c = sg("g1", pi=call == "sbn_msm_batch_check")
        add(call, "segmented", UNSUPPORTED, args={"kind": 1}, **c)
        add(call, "segmented", BAD_ARG, null=["lengths"], **c)
        add(call, "segmented", BAD_ARG, args={"segments": 0}, **c)
        add(call, "segmented", BAD_ARG, edits=[("lengths", [2], "set", 0)], **c)
        add(call, "segmented", BAD_ARG, edits=[("lengths", [1], "set", 1 << 60)], **c)
        add(call, "segmented", BAD_ARG, args={"start_count": 2}, **c)
        add(call, "segmented", BAD_ARG, args={"num_io": 0}, **c)
        add(call, "segmented", BAD_ARG, force_sums=True, **sg("fq", pi=call == "sbn_msm_batch_check"))
    add("sbn_msm_batch_instances", "segmented", BAD_ARG, null=["terms"], **sg("g2"))
    c = sg("fq12", pi=True)
    add("sbn_msm_batch_check", "segmented", BAD_ARG, null=["pi"], args={"units": 2}, **c)
    add("sbn_msm_batch_check", "segmented", VERIFY, args={"units": 1}, **c)
    add("sbn_msm_batch_check", "segmented", BAD_ARG, null_units=[1], **c)

    # ---- the constants
    for t in CURVES:
        add("sbn_curve_generator", "constant", OK, table=t)
    add("sbn_curve_generator", "constant", UNSUPPORTED, table="fq")
    add("sbn_curve_generator", "constant", UNSUPPORTED)
    add("sbn_curve_generator", "constant", BAD_ARG, table="g2", without=["out"])
    for call in ("sbn_g2_cofactor", "sbn_bn_x"):
        add(call, "constant", OK)
        add(call, "constant", BAD_ARG, without=["out"])
    return cases


def main():
    import starky_bn254_amd as S
    L = S.lib()
    recorded = []
    for case, want in _cases():
        rc, text, digests = run_case(L, case)
        assert rc == want, (case, rc, text)
        recorded.append(dict(case, rc=rc, error=text, sha256=digests))
    with open(OUT, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(recorded), "cases,", len({c["error"] for c in recorded}), "distinct texts ->", OUT)


if __name__ == "__main__":
    main()
