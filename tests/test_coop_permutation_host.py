"""sbn_poseidon_permute_coop_batch without a device: the entry is exported, and it refuses a null pointer and a non-canonical word
before it looks for a device, as the neighbouring building blocks refuse their arguments."""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
BAD_ARG, NON_CANONICAL = -1, -2


def test_coop_batch_refuses_bad_arguments_before_it_looks_for_a_device(S):
    L = S.lib()
    assert "sbn_poseidon_permute_coop_batch" in S.EXPORTS and hasattr(L, "sbn_poseidon_permute_coop_batch")
    assert L.sbn_poseidon_permute_coop_batch(None, 1) == BAD_ARG
    assert L.sbn_poseidon_permute_coop_batch(None, 0) == BAD_ARG
    st = np.zeros((3, 12), dtype=np.uint64)
    st[2, 7] = P                                         # word 2 * 12 + 7
    assert L.sbn_poseidon_permute_coop_batch(S.api._ptr(st), 3) == NON_CANONICAL
    assert b"state word 31 " in L.sbn_last_error()
    st[2, 7] = 2**64 - 1
    with pytest.raises(S.SbnError) as e:
        S.poseidon_permute_coop_batch(st)
    assert e.value.code == NON_CANONICAL
    assert st[2, 7] == 2**64 - 1                         # the caller's array is not written
