"""Shared by tests/test_check_trace_host.py, tests/test_check_trace_gpu.py and the column sweep (tests/column_sweep.py): the tables of the trace check at their smallest
height, the cells the tests change, and the independent reference -- the oracle's constraint-by-constraint evaluator
(orc_eval_constraints) applied on the trace domain H: L_first = [i == 0], L_last = [i == n - 1], z_last = g^i - g^(n - 1).
Traces and the oracle's verdict on the valid trace are built once per process."""
import functools

import numpy as np

import oracle_lib as O
import starky_bn254_amd as S

P = O.GL_P
ORACLE_ALPHAS = [0x1234567890ABCDEF, 0x0FEDCBA987654321]   # the oracle folds with its own: only "zero or not" is compared
NOPI = np.zeros(0, dtype=np.uint64)

SMALL_TABLES = ["g1op", "modular", "lookup", "flags", "flags_u64", "fq12exp", "fq12exp_u64"]   # 512 rows each


def _exp_start_lookups(stark, flag_cols, periodic):
    """First column of the range-check block of an Fq12 Exp table (csrc/air.cuh ExpShape): main columns, flags, the rotation
    pulse (counter, witness) where the table has one, the io-pulse counter and (witness, pulse) per block boundary."""
    return 108 * 16 + flag_cols + (2 if periodic else 0) + 1 + 4 * stark.num_io


def exp_ios(name):
    """The instances of the three 2^16-row Exp cases (128 each: the u16 range check needs that many rows), as the host and the
    device generators take them."""
    return {"g1exp": lambda: O.g1exp_inputs(128, 1), "g2exp": lambda: O.g2exp_inputs(128, 2), "fqexp": lambda: O.fqexp_inputs(128, 4)}[name]()[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """stark, valid trace (host generator), public inputs, and the three columns the tests change: one of the first gadget, one
    of the range check / lookup (the counter of the io pulses for the flag tables, which have neither), the last one."""
    if name == "g1op":
        stark = S.G1Stark()
        trace, pi = stark.generate_trace(O.g1op_inputs(512, 0)[0]), NOPI
        cols = (64 + 16, 386 + 1 + 2)              # new_x limb 0 of the add gadget; the sorted copy of range-check target 0
    elif name == "modular":
        stark = S.ModularStark()
        trace, pi = stark.generate_trace(O.modular_inputs(512, 6)[0]), NOPI
        cols = (2 * 16, 9 * 16 + 1 + 1 + 2)        # output limb 0 of the modular gadget; the sorted copy of target 0
    elif name == "modular_8192":
        stark = S.ModularStark()
        trace, pi = stark.generate_trace(O.modular_inputs(8192, 6)[0]), NOPI
        cols = (2 * 16, 9 * 16 + 1 + 1 + 2)
    elif name == "lookup":
        stark = S.MyStark()
        trace, pi = stark.generate_trace(*O.lookup_inputs(512, 9)), NOPI
        cols = (0, 2)                              # inputs; permuted inputs
    elif name == "flags":
        stark = S.FlagStark(1)
        trace, pi = stark.generate_trace(O.flags_inputs(1, 8)[0]), NOPI
        cols = (2, 16)                             # a flag column; the io-pulse counter
    elif name == "flags_u64":
        stark = S.FlagU64Stark(4)
        trace, pi = stark.generate_trace(O.flags_u64_inputs(4, 10)[0]), NOPI
        cols = (1, 6)
    elif name == "fq12exp":
        stark = S.Fq12ExpStark(1)
        trace, pi = stark.generate_trace_and_public_inputs(O.fq12exp_inputs(1, 3)[0])
        cols = (384, _exp_start_lookups(stark, 14, True) + 1 + 2)    # output coefficient 0 limb 0; the sorted copy of target 0
    elif name == "fq12exp_u64":
        stark = S.Fq12ExpU64Stark(4)
        trace, pi = stark.generate_trace_and_public_inputs(O.fq12expu64_inputs(4, 5)[0])
        cols = (384, _exp_start_lookups(stark, 6, False) + 1 + 2)
    elif name == "g1exp":
        stark = S.G1ExpStark(128)
        ios = O.g1exp_inputs(128, 1)[0]
        trace, pi = stark.generate_trace_and_public_inputs(ios)
        cols = (64 + 16, 384 + 14 + 2 + 1 + 4 * 128 + 2)             # new_x limb 0; the sorted copy of range-check target 0
    elif name == "fq12mul":
        stark = S.Fq12Stark()
        trace, pi = stark.generate_trace(O.fq12mul_inputs(512, 7)[0]), NOPI
        cols = (24 * 16, 108 * 16 + 1 + 1 + 2)     # output coefficient 0 limb 0; the sorted copy of target 0
    elif name == "g2exp":
        stark = S.G2ExpStark(128)
        trace, pi = stark.generate_trace_and_public_inputs(exp_ios(name))
        cols = (128 + 32, 768 + 14 + 2 + 1 + 4 * 128 + 2)            # new_x.c0 limb 0; the sorted copy of range-check target 0
    elif name == "fqexp":
        stark = S.FqExpStark(128)
        trace, pi = stark.generate_trace_and_public_inputs(exp_ios(name))
        cols = (32, 144 + 14 + 2 + 1 + 4 * 128 + 2)                  # output limb 0; the sorted copy of range-check target 0
    else:
        raise KeyError(name)
    n = trace.shape[1]
    cols = cols + (trace.shape[0] - 1,)
    assert all(0 <= c < trace.shape[0] for c in cols) and len(set(cols)) == 3
    rows = [0, 1, 255, 256, n - 1]                 # 255 | 256: the workgroup boundary of the kernels
    rpi = S.api._rows_per_instance(stark)
    if stark.kind in (S.AIR_G1_EXP, S.AIR_G2_EXP, S.AIR_FQ12_EXP, S.AIR_FQ_EXP, S.AIR_FQ12_EXP_U64):
        rows += [r for r in (rpi - 1, rpi, 511, 512) if r < n]       # the instance boundary, where the table has one
    rows = sorted(set(rows))
    trace.setflags(write=False)
    return {"name": name, "stark": stark, "trace": trace, "pi": pi, "cols": cols, "rows": rows, "n": n}


def corruptions(name):
    c = case(name)
    return [(r, col) for r in c["rows"] for col in c["cols"]]


def corrupt(trace, cells):
    """A copy with every (row, column) of `cells` changed to (v + 1) mod p."""
    bad = np.array(trace, dtype=np.uint64)
    for r, col in cells:
        bad[col, r] = (int(bad[col, r]) + 1) % P
    return bad


def oracle_nonzero(c, trace, rows=None):
    """[the oracle's accumulators are non-zero on row i] for i in rows (default: every row)."""
    n = c["n"]
    lg = n.bit_length() - 1
    g = pow(1753635133440165772, 1 << (32 - lg), P)
    g_last = pow(g, n - 1, P)
    rows = range(n) if rows is None else rows
    need = sorted({i for r in rows for i in (r, (r + 1) % n)})
    rowmajor = {i: np.ascontiguousarray(trace[:, i]) for i in need} if len(need) < n else None
    tt = np.ascontiguousarray(trace.T) if rowmajor is None else None
    out = {}
    for i in rows:
        lv, nv = (tt[i], tt[(i + 1) % n]) if tt is not None else (rowmajor[i], rowmajor[(i + 1) % n])
        acc = O.eval_constraints(c["stark"].kind, c["stark"].num_io, lv, nv, c["pi"], ORACLE_ALPHAS,
                                 (pow(g, i, P) - g_last) % P, int(i == 0), int(i == n - 1))
        out[i] = acc != [0, 0]
    return out


def consistent(report):
    """first_failing_row and the per-segment counts agree with the flags."""
    f = report.row_flags
    nz = np.nonzero(f)[0]
    assert report.rows == len(f) and report.failing_rows == len(nz)
    assert report.first_failing_row == (int(nz[0]) if len(nz) else None)
    assert report.ok == (len(nz) == 0)
    assert [s["name"] for s in report.segments] == ["air_head", "air_tail", "perm_lo", "perm_hi"]
    for s, seg in enumerate(report.segments):
        rows = np.nonzero(f & (1 << s))[0]
        assert seg["failing_rows"] == len(rows), seg
        assert seg["first_row"] == (int(rows[0]) if len(rows) else None), seg
    assert not (f >> 4).any()
