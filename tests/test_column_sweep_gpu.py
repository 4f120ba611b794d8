"""Every column of every table through the device trace check and explain: the packed copies of tests/column_sweep.py loaded
into one prover per table, and check_trace / explain_rows / explain_trace compared with their host forms on the same matrix and
seed, bit for bit.  (The host forms are held to the oracle and to numpy by tests/test_column_sweep_host.py.)  trace_check.hip
runs the prover's own quotient kernels on the trace domain, so a column those kernels misread shows here; afterwards the same
prover must still prove the valid trace word for word, and its proof of a packed copy equals the oracle's and is rejected."""
import time

import numpy as np
import pytest

import check_trace_cases as K
import column_sweep as W

pytestmark = pytest.mark.gpu
SEED = W.SEED
# Pass 0 alone for the four 512-row tables above 2,000 columns (19 and 78 copies); every pass for the rest (a 2^16-row table: one
# copy, so four uploads).
PASSES = {name: (1 if name in ("g1op", "fq12exp", "fq12exp_u64", "fq12mul") else W.PASSES) for name in W.TABLES}
LDE_TABLES = ("modular", "lookup", "flags", "fq12mul")


def _device(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)


def _accepted(S, O, stark, proof, cfg):
    """Both verifiers, which must agree: True / False."""
    oracle_ok = O.verify(stark.kind, stark.num_io, proof.words)[0] == 0
    try:
        S.verify_stark_proof(stark, proof, cfg)
        ours = True
    except S.SbnError as e:
        assert e.code == -6, e
        ours = False
    assert ours == oracle_ok
    return ours


def _same_check(S, prover, c, trace, who):
    dev = prover.check_trace(SEED, flags=True)
    host = S.check_trace_host(c["stark"], trace, c["pi"], seed=SEED, flags=True)
    K.consistent(dev)
    diff = np.nonzero(dev.row_flags != host.row_flags)[0]
    assert len(diff) == 0, f"{who}: row flags differ on rows {[int(i) for i in diff[:8]]}: device {[int(dev.row_flags[i]) for i in diff[:8]]}, host {[int(host.row_flags[i]) for i in diff[:8]]}"
    assert dev.segments == host.segments and dev.first_failing_row == host.first_failing_row and dev == host, who
    return dev


def _same_explain(S, prover, c, trace, rows, cells, who):
    dev_rows = prover.explain_rows(rows, SEED)
    host_rows = S.explain_rows_host(c["stark"], trace, c["pi"], rows, seed=SEED)
    for what, d, h in (("blocks", dev_rows.block_flags, host_rows.block_flags), ("Z flags", dev_rows.z_flags, host_rows.z_flags)):
        diff = np.nonzero((d != h).any(axis=1))[0]
        owner = W.cell_of_row(cells)
        assert len(diff) == 0, f"{who}: {what} differ on rows {[rows[i] for i in diff[:8]]}, (row, column) of the cells {[owner.get(rows[i]) for i in diff[:8]]}"
    dev, host = prover.explain_trace(SEED), S.explain_trace_host(c["stark"], trace, c["pi"], seed=SEED)
    for f in ("block_failing_rows", "block_first_row", "z_failing_rows", "z_first_row"):
        diff = np.nonzero(getattr(dev, f) != getattr(host, f))[0]
        assert len(diff) == 0, f"{who}: explain_trace {f} differs at {[int(i) for i in diff[:8]]}"
    return dev


@pytest.mark.parametrize("name", W.TABLES)
def test_every_column_device_equals_host(S, O, name):
    _device(S)
    c = K.case(name)
    stark, n, pi = c["stark"], c["n"], c["pi"]
    cfg = stark.config()
    prover = S.Prover(stark, cfg, n.bit_length() - 1)
    if name in W.DEVICE_WITNESS:                    # sweep what the device generator wrote; it equals the host generator's
        assert np.array_equal(prover.generate_trace(K.exp_ios(name)), pi)
        valid = prover.read_trace()
        assert np.array_equal(valid, c["trace"]), f"{name}: device witness differs from the host generator's in columns {np.nonzero((valid != c['trace']).any(axis=1))[0][:8]}"
    else:
        valid = c["trace"]
        prover.load_trace(valid, pi)
    before = prover.prove()
    t0 = time.perf_counter()
    first_copy = None
    for p in range(PASSES[name]):
        for k, (cells, bad) in enumerate(W.copies(valid, p)):
            who = f"{name} pass {p} copy {k}"
            prover.load_trace(bad, pi)
            rep = _same_check(S, prover, c, bad, who)
            assert not rep.ok, who
            _same_explain(S, prover, c, bad, W.touched_rows(cells), cells, who)
            assert np.array_equal(prover.read_trace(), bad), who
            if first_copy is None and name in LDE_TABLES:
                first_copy = bad
            del bad
    sweep_seconds = time.perf_counter() - t0

    # the valid trace again, through the same prover: nothing of a check stays behind in the buffers prove() shares with it
    prover.load_trace(valid, pi)
    rep = _same_check(S, prover, c, valid, f"{name} valid")
    assert rep.ok and not rep.row_flags.any()
    assert _same_explain(S, prover, c, valid, [0, 1, n - 1], (), f"{name} valid").ok
    after = prover.prove()
    assert np.array_equal(before.words, after.words), f"{name}: the proof of the valid trace changed after the sweep"

    # the listed free columns: the hole is the reference AIR's, not the check's -- both verifiers accept the proof
    for col in W.FREE_COLUMNS.get(name, []):
        cell = (W.cell_row(n, col % ((n - 8) // 4), 0), col)
        bad = W.one_cell(valid, cell)
        prover.load_trace(bad, pi)
        rep = _same_check(S, prover, c, bad, f"{name} free column {col}")
        assert rep.ok and not rep.row_flags.any(), (name, cell, str(rep))
        proof = prover.prove()
        assert not np.array_equal(proof.words, before.words)
        assert _accepted(S, O, stark, proof, cfg), (name, cell)

    # an invalid trace on the LDE: the quotient of the first packed copy, word for word the oracle's, and rejected
    if name in LDE_TABLES:
        prover.load_trace(first_copy, pi)
        proof = prover.prove()
        ref, _ = O.prove(stark.kind, stark.num_io, first_copy, pi)
        diff = np.nonzero(proof.words != ref)[0] if len(proof.words) == len(ref) else [-1]
        assert len(diff) == 0, f"{name}: proof of the first packed copy differs from the oracle's, first at word {int(diff[0])}"
        assert not _accepted(S, O, stark, proof, cfg), name
    prover.close()
    print(f"{name}: {PASSES[name]} pass(es), sweep {sweep_seconds:.1f} s")
