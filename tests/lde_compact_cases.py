"""What tests/test_lde_compact_host.py (CPU: the interface, the refusals and the memory plan) and tests/test_lde_compact_gpu.py
(device: rows from coefficients and whole proofs of compact contexts) share.  The tables, config rows and oracle proofs are those of
tests/rate_cases.py and tests/rate_oracle.py, the digests those of tests/golden/rate3_digests.json."""
import ctypes as C

import numpy as np

P = 0xFFFFFFFF00000001
RING_DEPTH = 2   # slots of the LDE chunk ring (csrc/prover_ctx.hpp LDE_RING_DEPTH)


def bitrev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def ntt_chunk(degree_bits, rate_bits):
    """Columns per chunk of the commit pipeline at rate_bits > 1 (csrc/prover.hip ctx_shape): 64, 48 from 2^18 LDE rows up."""
    assert rate_bits > 1
    return 48 if degree_bits + rate_bits >= 18 else 64


def big_columns(stark, cfg):
    """Column counts of the matrices a compact context thins out: those of more than 4 columns."""
    return [c for c in (stark.num_columns, stark.num_permutation_zs(cfg)) if c > 4]


def ring_bytes(degree_bits, rate_bits):
    return RING_DEPTH * ntt_chunk(degree_bits, rate_bits) * (8 << (degree_bits + rate_bits))


def expected_saving(stark, cfg, degree_bits):
    """plan(full) - plan(compact) by the arithmetic of the issue: every wide column keeps qn = 2n of its m rows, the ring is added."""
    big = big_columns(stark, cfg)
    if not big:
        return 0
    n = 1 << degree_bits
    m, qn = n << cfg.rate_bits, 2 * n
    return 8 * sum(big) * (m - qn) - ring_bytes(degree_bits, cfg.rate_bits)


def options(struct_size=None, lde_storage=0):
    from starky_bn254_amd.api import _ProverOptions
    return _ProverOptions(C.sizeof(_ProverOptions) if struct_size is None else struct_size, lde_storage)


def raw_plan(S, stark, cfg, degree_bits, opt):
    """(code, bytes, message) of sbn_prover_memory_plan with an options struct passed as it is."""
    out = C.c_uint64(0)
    rc = S.lib().sbn_prover_memory_plan(C.byref(stark._d), C.byref(cfg._c), degree_bits, C.byref(opt) if opt is not None else None, C.byref(out))
    return rc, int(out.value), S.lib().sbn_last_error().decode() if rc else ""


def raw_create(S, stark, cfg, degree_bits, opt):
    """(code, message) of sbn_prover_create_with for arguments it must refuse; a context that is created after all is destroyed."""
    h = C.c_void_p()
    rc = S.lib().sbn_prover_create_with(C.byref(stark._d), C.byref(cfg._c), degree_bits, C.byref(opt) if opt is not None else None, C.byref(h))
    msg = S.lib().sbn_last_error().decode() if rc else ""
    if h.value:
        S.lib().sbn_prover_destroy(h)
    return rc, msg


def root_of_unity(bits):
    return pow(7, (P - 1) >> bits, P)


def column_of_top_coefficient(n, c):
    """Values over the trace domain of the polynomial c X^(n-1): c w^(-i)."""
    w_inv = pow(root_of_unity(n.bit_length() - 1), P - 2, P)
    out, v = np.zeros(n, dtype=np.uint64), c % P
    for i in range(n):
        out[i] = v
        v = v * w_inv % P
    return out
