"""The batch verifier's interface without a device: the entry points exist, and sbn_verifier_create answers everything it can
answer before it looks for a device -- config_supported(), the table and degree_bits checks, as sbn_prover_create does -- and
SBN_ERR_NO_DEVICE after that (no fallback: sbn_verify is the host verifier).  The verdicts themselves are compared with the host
verifier's in test_verifier_gpu.py."""
import ctypes as C

import pytest

ENTRY_POINTS = ["sbn_verifier_create", "sbn_verifier_verify", "sbn_verifier_reason", "sbn_verifier_destroy"]


def create_code(S, stark, cfg, degree_bits, max_batch=4):
    try:
        v = S.Verifier(stark, cfg, degree_bits, max_batch)
    except S.SbnError as e:
        return e.code
    v.close()
    return 0


def test_entry_points_exist(S):
    L = S.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in S.EXPORTS, name
    assert callable(S.Verifier) and hasattr(S.Verifier, "verify") and hasattr(S.Verifier, "close")


@pytest.mark.parametrize("field,value", [("num_challenges", 1), ("num_challenges", 3), ("rate_bits", 0), ("rate_bits", 2), ("cap_height", 0),
                                         ("cap_height", 9), ("fri_arity_bits", 0), ("fri_arity_bits", 5), ("num_query_rounds", 0),
                                         ("num_query_rounds", 513), ("proof_of_work_bits", 33), ("fri_variant", 3)])
def test_unsupported_config_values_are_refused(S, field, value):
    stark = S.G1Stark()
    cfg = stark.config()
    setattr(cfg, field, value)
    assert create_code(S, stark, cfg, 9) == -7


def test_unknown_table_and_zero_batch_are_bad_arguments(S):
    stark = S.G1Stark()
    d = S.api._AirDesc(99, 0)
    h = C.c_void_p()
    assert S.lib().sbn_verifier_create(C.byref(d), C.byref(stark.config()._c), 9, 4, C.byref(h)) == -1
    assert not h.value
    assert create_code(S, stark, stark.config(), 9, max_batch=0) == -1


@pytest.mark.parametrize("degree_bits", [8, 23])
def test_degree_bits_outside_9_to_22_are_refused(S, degree_bits):
    assert create_code(S, S.G1Stark(), S.G1Stark().config(), degree_bits) == -7


def test_null_out_is_a_bad_argument(S):
    stark = S.G1Stark()
    assert S.lib().sbn_verifier_create(C.byref(stark._d), C.byref(stark.config()._c), 9, 4, None) == -1


def test_a_supported_create_needs_a_device(S):
    if S.lib().sbn_device_count() > 0:
        v = S.Verifier(S.G1Stark(), S.G1Stark().config(), 9, 4)   # on a GPU machine the same call succeeds
        v.close()
        return
    assert create_code(S, S.G1Stark(), S.G1Stark().config(), 9) == -3
    assert "sbn_verify is the host verifier" in S.lib().sbn_last_error().decode()


def test_null_handles_are_harmless(S):
    L = S.lib()
    L.sbn_verifier_destroy(None)
    assert L.sbn_verifier_reason(None, 0) == b""
    out = (C.c_int32 * 1)(77)
    assert L.sbn_verifier_verify(None, None, None, 1, out) == -1 and out[0] == 77
