"""Verified proving on the device (include/sbn.h sbn_prover_set_guard): a guarded context returns the words of the unguarded call
when they verify, and SBN_ERR_VERIFY_FAILED with the verifier's own reason -- the text sbn_verify leaves for the proof the unguarded
call hands out -- when they do not, with the trace still loaded for the diagnostics.  Tables: LookupStark at 2^9 rows (two Z
columns, rows are their own leaves), FlagStark(2) at 2^10 (no Z commitment), Fq12ExpU64Stark(4) at 2^9 (the smallest Exp table,
device witness); configs: standard_fast_config and rate_bits 3; both modes.  The bad traces are valid traces with one main-column
cell incremented mod p, taken from the candidates of tests/check_trace_cases.py; a candidate the trace check does not flag is
replaced by the next one."""
import ctypes as C
import functools

import numpy as np
import pytest

import check_trace_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu
SEED = 0x9E3779B97F4A7C15
VERIFY_FAILED, UNSUPPORTED, BAD_ARG = -6, -7, -1
TABLES = ["lookup", "flags2", "fq12exp_u64"]
CONFIGS = ["fast", "rate3"]
MODES = ["device", "host"]


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    S.lib().sbn_set_device(0)
    return S


@functools.lru_cache(maxsize=None)
def table(name):
    """stark, valid host trace, public inputs, the instance list where the table has a device witness, and the main-column cells
    a bad trace is made from."""
    import starky_bn254_amd as S
    if name == "flags2":
        stark = S.FlagStark(2)
        trace = stark.generate_trace(O.flags_inputs(2, 8)[0])
        trace.setflags(write=False)
        t = {"stark": stark, "trace": trace, "pi": K.NOPI, "col": K.case("flags")["cols"][0], "rows": [1, 0, 255, 256, 511, 512, 1023]}
    else:
        c = K.case(name)
        t = {"stark": c["stark"], "trace": c["trace"], "pi": c["pi"], "col": c["cols"][0], "rows": [1] + [r for r in c["rows"] if r != 1]}
    t["ios"] = O.fq12expu64_inputs(4, 5)[0] if name == "fq12exp_u64" else None
    t["bits"] = t["trace"].shape[1].bit_length() - 1
    assert t["trace"].shape == (t["stark"].num_columns, {"lookup": 512, "flags2": 1024, "fq12exp_u64": 512}[name])
    return t


def config(S, t, which):
    return t["stark"].config() if which == "fast" else S.StarkConfig.for_rate(3)


def load_valid(p, t):
    if t["ios"] is not None:
        p.generate_trace(t["ios"])     # the device witness
    else:
        p.load_trace(t["trace"], t["pi"])


_BAD = {}


def bad_trace(p, name):
    """The valid trace with one main-column cell incremented, loaded into `p`: the first candidate cell whose trace the trace check
    flags (found once per table), and the report."""
    t = table(name)
    cells = [_BAD[name]] if name in _BAD else [(r, t["col"]) for r in t["rows"]]
    for cell in cells:
        bad = K.corrupt(t["trace"], [cell])
        p.load_trace(bad, t["pi"])
        rep = p.check_trace(SEED)
        if not rep.ok:
            _BAD[name] = cell
            return bad, rep
    pytest.fail(f"{name}: the trace check flags none of the candidate cells {cells}")


def host_verdict(S, stark, cfg, proof):
    b = proof.to_bytes()
    buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
    rc = S.lib().sbn_verify(C.byref(stark._d), C.byref(cfg._c), buf, len(b))
    return rc, (S.lib().sbn_last_error().decode() if rc else "")


def check_stats(st, checked, rejected, mode):
    assert (st.checked, st.rejected) == (checked, rejected) and st.ns > 0, st
    assert (st.device_bytes > 0) == (mode == "device"), st


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", CONFIGS)
@pytest.mark.parametrize("name", TABLES)
def test_valid_trace_same_words_and_stats(gpu, name, which, mode):
    S, t = gpu, table(name)
    cfg = config(S, t, which)
    p = S.Prover(t["stark"], cfg, t["bits"])
    try:
        load_valid(p, t)
        assert p.guard_stats() == (0, 0, 0, 0)
        want = p.prove().words
        assert host_verdict(S, t["stark"], cfg, S.Proof(want, t["bits"])) == (0, "")
        p.set_guard(mode)
        p.set_guard(mode)                       # the mode it already has: nothing changes
        assert p.guard_stats() == (0, 0, 0, 0)  # the verifier is created by the first guarded proof
        for k in (1, 2):                        # the second proof: the trace is still loaded
            assert np.array_equal(p.prove().words, want)
            check_stats(p.guard_stats(), k, 0, mode)
        after = p.guard_stats()
        p.set_guard(None)                       # off again: the same words, nothing counted, the verifier stays
        assert np.array_equal(p.prove().words, want)
        assert p.guard_stats() == after
    finally:
        p.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", CONFIGS)
@pytest.mark.parametrize("name", TABLES)
def test_bad_cell_is_refused_with_the_verifiers_reason(gpu, name, which, mode):
    S, t = gpu, table(name)
    L = S.lib()
    cfg = config(S, t, which)
    p = S.Prover(t["stark"], cfg, t["bits"])
    try:
        bad, rep0 = bad_trace(p, name)
        rc, reason = host_verdict(S, t["stark"], cfg, p.prove())   # unguarded: a proof comes back, and no verifier accepts it
        assert rc == VERIFY_FAILED and reason
        p.set_guard(mode)
        with pytest.raises(S.SbnError) as e:
            p.prove()
        assert e.value.code == VERIFY_FAILED and e.value.reason == reason
        check_stats(p.guard_stats(), 1, 1, mode)
        h = C.c_void_p(1)                                          # the C call: the status, the message, and no proof object
        assert L.sbn_prover_prove(p._h, C.byref(h)) == VERIFY_FAILED and h.value is None and L.sbn_last_error().decode() == reason
        check_stats(p.guard_stats(), 2, 2, mode)
        assert p.check_trace(SEED) == rep0 and not rep0.ok         # the trace stays loaded for the diagnostics
        assert np.array_equal(p.read_trace(), bad)
        load_valid(p, t)                                           # the same context proves and verifies again
        good = p.prove()
        assert host_verdict(S, t["stark"], cfg, good) == (0, "")
        check_stats(p.guard_stats(), 3, 2, mode)
        p.set_guard(None)
        assert np.array_equal(p.prove().words, good.words)
    finally:
        p.close()


@pytest.mark.parametrize("call", ["host_trace", "host_columns", "host_rows"])
def test_load_and_prove_calls(gpu, call):
    """prove_host_trace / prove_host_columns / prove_host_rows on LookupStark under the device guard: the words of the unguarded
    proof for the valid trace; for the bad one -6 with the verifier's reason, and -- unlike every other failure of these calls --
    the trace stays loaded."""
    S, t = gpu, table("lookup")
    cfg = t["stark"].config()

    def run(p, trace):
        if call == "host_trace":
            return p.prove_host_trace(trace, t["pi"])
        if call == "host_columns":
            return p.prove_host_columns([np.ascontiguousarray(c) for c in trace], t["pi"])
        return p.prove_host_rows(np.ascontiguousarray(trace.T), t["pi"])

    p = S.Prover(t["stark"], cfg, 9)
    try:
        bad, rep0 = bad_trace(p, "lookup")
        rc, reason = host_verdict(S, t["stark"], cfg, run(p, bad))
        assert rc == VERIFY_FAILED and reason
        want = run(p, t["trace"]).words
        p.set_guard("device")
        assert np.array_equal(run(p, t["trace"]).words, want)
        check_stats(p.guard_stats(), 1, 0, "device")
        assert np.array_equal(p.prove().words, want)               # resident as after the unguarded call
        with pytest.raises(S.SbnError) as e:
            run(p, bad)
        assert e.value.code == VERIFY_FAILED and e.value.reason == reason
        check_stats(p.guard_stats(), 3, 1, "device")
        assert p.check_trace(SEED) == rep0 and np.array_equal(p.read_trace(), bad)
        assert np.array_equal(run(p, t["trace"]).words, want)
    finally:
        p.close()


def _units(S, count):
    """`count` units of Fq12ExpU64Stark(4): instance lists, host traces and public inputs."""
    stark = S.Fq12ExpU64Stark(4)
    ios = [O.fq12expu64_inputs(4, 5 + u)[0] for u in range(count)]
    tp = [stark.generate_trace_and_public_inputs(i) for i in ios]
    return stark, np.stack(ios), [x[0] for x in tp], [x[1] for x in tp]


@pytest.mark.parametrize("inflight,count", [(2, 2), (1, 3)])
def test_batch(gpu, inflight, count):
    """The guarded batch prover: prove_ios gives the unguarded batch's words; a bad cell in the last unit of prove_host_traces fails
    the call with -6 behind "unit <u>: ", every proof slot null, and the batch prover stays usable."""
    S = gpu
    L = S.lib()
    stark, ios, traces, pis = _units(S, count)
    cfg = stark.config()
    plain = S.BatchProver(stark, cfg, 9, inflight=inflight)
    try:
        want = [pr.words for pr in plain.prove_ios(ios)]
    finally:
        plain.close()
    single = S.Prover(stark, cfg, 9)
    try:
        single.load_trace(traces[0], pis[0])                       # (a context to find the cell with; unit 0 is K.case's trace)
        assert np.array_equal(traces[0], table("fq12exp_u64")["trace"])
        bad_trace(single, "fq12exp_u64")
        cell = _BAD["fq12exp_u64"]
        bad = K.corrupt(traces[count - 1], [cell])
        single.load_trace(bad, pis[count - 1])
        assert not single.check_trace(SEED).ok
        rc, reason = host_verdict(S, stark, cfg, single.prove())
        assert rc == VERIFY_FAILED
    finally:
        single.close()
    bp = S.BatchProver(stark, cfg, 9, inflight=inflight, guard="device")
    try:
        got = bp.prove_ios(ios)
        assert len(got) == count and all(np.array_equal(g.words, w) for g, w in zip(got, want))
        st = bp.guard_stats()
        assert (st.checked, st.rejected) == (count, 0) and st.ns > 0 and st.device_bytes > 0
        units = traces[:count - 1] + [bad]
        tables = [S.ColumnTable(np.ascontiguousarray(u)) for u in units]
        addr = np.concatenate([tb.addr for tb in tables])
        pi_addr = np.array([q.ctypes.data for q in pis], dtype=np.uint64)
        out = (C.c_void_p * count)(*([1] * count))
        rc = L.sbn_batch_prover_prove_host_columns(bp._h, addr.ctypes.data_as(C.c_void_p), stark.num_columns, 0, pi_addr.ctypes.data_as(C.c_void_p),
                                                   stark.num_public_inputs, count, out)
        msg = L.sbn_last_error().decode()
        assert rc == VERIFY_FAILED and msg == f"unit {count - 1}: {reason}", (rc, msg)
        assert all(h is None for h in out)
        with pytest.raises(S.SbnError) as e:
            bp.prove_host_traces(units, pis)
        assert e.value.code == VERIFY_FAILED and e.value.reason.startswith(f"unit {count - 1}: ")
        assert bp.guard_stats().rejected == 2
        got = bp.prove_host_traces(traces, pis)                     # usable, and the valid units verify
        assert all(np.array_equal(g.words, w) for g, w in zip(got, want))
    finally:
        bp.close()


def test_one_shot(gpu):
    """prove() under prove_set_guard("device") with a cache that holds the context and its verifier: the verifier's bytes count
    against the budget; a bad trace is -6 and its context is not kept; prove_set_guard(None) restores the unguarded call."""
    S, t = gpu, table("lookup")
    stark, cfg = t["stark"], t["stark"].config()
    p = S.Prover(stark, cfg, 9, guard="device")
    try:
        bad, _ = bad_trace(p, "lookup")
        p.set_guard(None)
        rc, reason = host_verdict(S, stark, cfg, p.prove())
        assert rc == VERIFY_FAILED
        p.set_guard("device")
        want = p.prove_host_trace(t["trace"], t["pi"]).words
        guard_bytes = p.guard_stats().device_bytes
    finally:
        p.close()
    plan = S.prover_memory_plan(stark, cfg, 9)
    assert guard_bytes > 0
    try:
        S.prove_cache_configure(plan + guard_bytes + (1 << 20))
        S.prove_set_guard("device")
        st0 = S.prove_cache_stats()                                 # (the counters are the process's: other tests have used the cache)
        for _ in range(2):                                          # a miss, then a hit on the context that owns the verifier
            assert np.array_equal(S.prove(stark, cfg, t["trace"], t["pi"]).words, want)
        st = S.prove_cache_stats()
        assert (st["hits"] - st0["hits"], st["misses"] - st0["misses"], st["contexts_resident"]) == (1, 1, 1)
        assert plan + guard_bytes <= st["bytes_resident"] <= plan + guard_bytes + 64, (st, plan, guard_bytes)
        with pytest.raises(S.SbnError) as e:
            S.prove(stark, cfg, bad, t["pi"])
        assert e.value.code == VERIFY_FAILED and e.value.reason == reason
        assert S.prove_cache_stats()["contexts_resident"] == 0     # a context whose call failed is not kept
        S.prove_set_guard(None)
        proof = S.prove(stark, cfg, bad, t["pi"])                   # today's behaviour: a proof that no verifier accepts
        assert host_verdict(S, stark, cfg, proof) == (VERIFY_FAILED, reason)
    finally:
        S.prove_set_guard(None)
        S.prove_cache_configure(0)


def test_split_prover_refuses(gpu):
    from starky_bn254_amd import split
    S = gpu
    c = K.case("fq12exp")
    stark, cfg = c["stark"], c["stark"].config()
    sb, rb = split.exchange_bytes(stark, cfg, 9, 1)
    grp = split.LocalGroup(1, sb, rb)
    p = split.SplitProver(stark, cfg, 9, transport=grp.comms[0])
    try:
        for mode in ("device", "host"):
            with pytest.raises(S.SbnError) as e:
                p.set_guard(mode)
            assert e.value.code == UNSUPPORTED, e.value
        with pytest.raises(S.SbnError) as e:
            p.set_guard(3)
        assert e.value.code == BAD_ARG
        p.load_trace(c["trace"], c["pi"])                           # and the context proves as before
        S.verify_stark_proof(stark, p.prove(), cfg)
    finally:
        p.close()
        grp.close()


def test_describe(gpu):
    S, t = gpu, table("lookup")
    p = S.Prover(t["stark"], t["stark"].config(), 9)
    try:
        fresh = p.describe()
        assert fresh["guard"] == "off" and fresh["guard_bytes"] == "0"
        p.load_trace(t["trace"], t["pi"])
        p.set_guard("device")
        assert p.describe()["guard"] == "device" and p.describe()["guard_bytes"] == "0"
        p.prove()
        d = p.describe()
        assert d["guard"] == "device" and int(d["guard_bytes"]) == p.guard_stats().device_bytes > 0
        assert list(d) == list(fresh)                               # every key stays, in place
        assert {k: v for k, v in d.items() if k not in ("guard", "guard_bytes")} == {k: v for k, v in fresh.items() if k not in ("guard", "guard_bytes")}
        assert int(d["dev_bytes"]) == S.prover_memory_plan(t["stark"], t["stark"].config(), 9)   # the guard is outside the plan
        p.set_guard("host")
        assert p.describe()["guard"] == "host" and p.describe()["guard_bytes"] == d["guard_bytes"]
    finally:
        p.close()
