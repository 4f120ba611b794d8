"""Verified proving (include/sbn.h sbn_prover_set_guard), the parts that need no device: the six functions are declared, exported
and bound; the Rust declarations list the five a Rust caller reaches; the refusals that come in front of any device work -- a
null handle, an unknown mode -- come back on a machine without a GPU; and a refused mode leaves the one-shot calls as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["sbn_prover_set_guard", "sbn_batch_prover_set_guard", "sbn_prove_set_guard", "sbn_prover_guard_stats", "sbn_batch_prover_guard_stats",
         "sbn_split_prover_set_guard"]
BAD_ARG = -1
OFF, DEVICE, HOST = 0, 1, 2


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sbn.h")).read(), flags=re.S)


def test_header_declares_and_library_exports(S):
    hdr = _header()
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
        assert hasattr(S.lib(), f) and f in S.EXPORTS, f
    m = re.search(r"enum \{ SBN_GUARD_OFF = (\d+), SBN_GUARD_DEVICE = (\d+), SBN_GUARD_HOST = (\d+) \};", hdr)
    assert m and [int(v) for v in m.groups()] == [OFF, DEVICE, HOST]
    assert S.GUARD == {None: OFF, "off": OFF, "device": DEVICE, "host": HOST}
    assert re.search(r"#define SBN_ABI_VERSION 4\b", hdr) and S.lib().sbn_abi_version() == 4
    # no existing struct changed: the options keep their size
    assert C.sizeof(S.api._ProverOptions) == 8 and re.search(r"typedef struct sbn_prover_options \{ uint32_t struct_size; uint32_t lde_storage; \}", hdr)


def test_rust_declarations_and_shim():
    shim = os.path.join(ROOT, "integration", "rust", "starky-bn254-amd", "src")
    ffi = open(os.path.join(shim, "ffi.rs")).read()
    for f in FUNCS[:5]:   # (the shim has no split prover)
        assert re.search(r"pub fn %s\(" % f, ffi), f
    for name, v in (("OFF", OFF), ("DEVICE", DEVICE), ("HOST", HOST)):
        assert "pub const SBN_GUARD_%s: u32 = %d;" % (name, v) in ffi
    lib_rs = open(os.path.join(shim, "lib.rs")).read()
    assert "pub fn set_guard" in lib_rs and "pub fn prove_ios_verified" in lib_rs and "run_once" in lib_rs


def _last(S):
    return S.lib().sbn_last_error().decode()


def test_refusals_without_a_device(S):
    L = S.lib()
    out = (C.c_uint64 * 4)()
    for mode in (3, 0xFFFFFFFF):
        assert L.sbn_prove_set_guard(mode) == BAD_ARG and "unknown guard mode" in _last(S)
    for mode in (OFF, DEVICE, HOST, 3):   # a null handle is refused first, whatever the mode
        for f in ("sbn_prover_set_guard", "sbn_batch_prover_set_guard", "sbn_split_prover_set_guard"):
            assert getattr(L, f)(None, mode) == BAD_ARG and _last(S) == "null argument", (f, mode)
    for f in ("sbn_prover_guard_stats", "sbn_batch_prover_guard_stats"):
        assert getattr(L, f)(None, out) == BAD_ARG and _last(S) == "null argument", f
    with pytest.raises(S.SbnError) as e:
        S.prove_set_guard(3)
    assert e.value.code == BAD_ARG and e.value.reason == _last(S)
    for bad in ("dev", "HOST", ""):
        with pytest.raises(ValueError):
            S.prove_set_guard(bad)
    S.prove_set_guard(None)


def _refused_one_shot_calls(S):
    """(rc, message) of one-shot calls that are refused before a device is looked for: an unsupported config, and a row-major
    trace of the wrong height."""
    stark = S.LookupStark()
    cfg = stark.config()
    cfg.rate_bits = 2
    trace = np.zeros((4, 512), dtype=np.uint64)
    got = []
    for call in (lambda: S.prove(stark, cfg, trace, np.zeros(0, dtype=np.uint64)),
                 lambda: S.prove_rows(stark, stark.config(), np.zeros((500, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint64))):
        with pytest.raises(S.SbnError) as e:
            call()
        got.append((e.value.code, e.value.reason))
    return got


def test_off_after_a_refusal_leaves_the_one_shot_calls_as_they_were(S):
    L = S.lib()
    before = _refused_one_shot_calls(S)
    assert before[0][0] == -7 and before[1][0] == BAD_ARG
    assert L.sbn_prove_set_guard(0xFFFFFFFF) == BAD_ARG
    assert L.sbn_prove_set_guard(OFF) == 0
    assert _refused_one_shot_calls(S) == before
    # and setting a mode looks for no device either: it only takes effect in the next call that proves
    for mode in (DEVICE, HOST, OFF):
        assert L.sbn_prove_set_guard(mode) == 0
    assert _refused_one_shot_calls(S) == before
