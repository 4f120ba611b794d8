"""Compact LDE storage without a device: the new entry points, their refusals (which all come before a device is looked for) and
sbn_prover_memory_plan held to the arithmetic of the buffers it drops and adds.  The device side is tests/test_lde_compact_gpu.py."""
import ctypes as C
import os
import re

import pytest

import lde_compact_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sbn_prover_create_with", "sbn_batch_prover_create_with", "sbn_prover_memory_plan", "sbn_lde_rows"]


def test_new_entry_points_are_declared_exported_and_bound(S):
    hdr = open(os.path.join(ROOT, "include", "sbn.h")).read()
    declared = set(re.findall(r"\b(sbn_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in S.EXPORTS and hasattr(S.lib(), name), name
    assert re.search(r"enum \{ SBN_LDE_FULL = 0, SBN_LDE_COMPACT = 1 \};", hdr)
    assert re.search(r"typedef struct sbn_prover_options \{ uint32_t struct_size; uint32_t lde_storage; \} sbn_prover_options;", hdr)
    assert S.LDE_STORAGE == {"full": 0, "compact": 1}
    assert S.lib().sbn_abi_version() == int(re.search(r"#define SBN_ABI_VERSION (\d+)", hdr).group(1))
    # the Rust shim declares them with the header's argument counts (test_product_host compares the counts of what it declares)
    ffi = open(os.path.join(ROOT, "integration", "rust", "starky-bn254-amd", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "pub struct sbn_prover_options" in ffi
    assert "pub fn with_options" in open(os.path.join(ROOT, "integration", "rust", "starky-bn254-amd", "src", "lib.rs")).read()


def test_python_names_of_the_storage_modes(S):
    with pytest.raises(ValueError):
        S.prover_memory_plan(S.G1Stark(), S.StarkConfig.for_rate(3), 9, lde="dense")


def test_refusals_come_in_header_order_without_a_device(S):
    """Bad struct_size, then an unknown mode, then compact at rate 1 -- each from sbn_prover_create_with, sbn_batch_prover_create_with
    and sbn_prover_memory_plan alike, on a machine with or without a GPU."""
    stark, c1, c3 = S.G1Stark(), S.StarkConfig(), S.StarkConfig.for_rate(3)
    size = C.sizeof(LC.options())
    assert size == 8

    def batch(cfg, opt):
        h = C.c_void_p()
        rc = S.lib().sbn_batch_prover_create_with(C.byref(stark._d), C.byref(cfg._c), 9, 2, C.byref(opt), C.byref(h))
        assert not h.value
        return rc, S.lib().sbn_last_error().decode()

    for call in (lambda cfg, opt: LC.raw_create(S, stark, cfg, 9, opt), lambda cfg, opt: LC.raw_plan(S, stark, cfg, 9, opt)[::2], batch):
        # a wrong size wins over an unknown mode, an unknown mode over the rate
        for cfg in (c1, c3):
            rc, msg = call(cfg, LC.options(struct_size=size + 4, lde_storage=7))
            assert rc == -1 and "struct_size" in msg, msg
            rc, msg = call(cfg, LC.options(struct_size=0, lde_storage=1))
            assert rc == -1 and "struct_size" in msg, msg
            rc, msg = call(cfg, LC.options(lde_storage=2))
            assert rc == -1 and "lde_storage" in msg, msg
        rc, msg = call(c1, LC.options(lde_storage=1))
        assert rc == -7 and "qn = m" in msg and "nothing would be dropped" in msg, msg
    # what sbn_prover_create refuses is refused as before, with options or without
    bad = S.StarkConfig.for_rate(2)
    assert LC.raw_plan(S, stark, bad, 9, LC.options(lde_storage=1))[0] == -7
    assert LC.raw_plan(S, stark, bad, 9, None)[0] == -7
    assert LC.raw_plan(S, stark, c3, 8, LC.options(lde_storage=1))[0] == -7            # height
    assert LC.raw_plan(S, S.G1ExpStark(128), c3, 15, None)[0] == -1                  # 512 * num_io rows
    idx, out = (C.c_uint32 * 1)(0), (C.c_uint64 * 2)()
    cols = (C.c_uint64 * 1024)()
    assert S.lib().sbn_lde_rows(cols, 2, 9, 3, idx, 0, out) == -1 and S.lib().sbn_lde_rows(cols, 2, 9, 3, idx, 65537, out) == -1   # count
    with pytest.raises(S.SbnError) as e:
        S.Prover(stark, c1, 9, lde="compact")
    assert e.value.code == -7
    with pytest.raises(S.SbnError) as e:
        S.BatchProver(S.Fq12ExpU64Stark(16), c1, 11, inflight=2, lde="compact")
    assert e.value.code == -7


def plan_tables(S):
    return [("G1Stark 2^9", S.G1Stark(), 9), ("FlagStark(8)", S.FlagStark(8), 12), ("G1ExpStark(128)", S.G1ExpStark(128), 16),
            ("Fq12ExpStark(16)", S.Fq12ExpStark(16), 13)]


def test_plan_difference_is_the_dropped_rows_minus_the_ring(S):
    """plan(full) - plan(compact) == 8 * sum over the wide matrices of cols * (m - qn) - ring bytes, the ring from the chunk rule."""
    cfg = S.StarkConfig.for_rate(3)
    for name, stark, bits in plan_tables(S):
        full, compact = S.prover_memory_plan(stark, cfg, bits, lde="full"), S.prover_memory_plan(stark, cfg, bits, lde="compact")
        big = LC.big_columns(stark, cfg)
        assert big and big[0] == stark.num_columns, name
        assert full - compact == LC.expected_saving(stark, cfg, bits), (name, full, compact)
        # (a table narrower than the ring pays for it: FlagStark(8) has 49 columns against 2 slots of 48)
        assert (compact < full) == (name != "FlagStark(8)"), name
    # FlagStark has no Z columns: only the trace is thinned out
    assert LC.big_columns(S.FlagStark(8), cfg) == [S.FlagStark(8).num_columns]
    assert len(LC.big_columns(S.G1Stark(), cfg)) == 2


def test_plan_of_a_table_that_stays_whole(S):
    cfg = S.StarkConfig.for_rate(3)
    for bits in (9, 14):
        assert S.prover_memory_plan(S.LookupStark(), cfg, bits, lde="full") == S.prover_memory_plan(S.LookupStark(), cfg, bits, lde="compact") > 0


def test_full_plan_is_the_plan_without_options(S):
    for name, stark, bits in plan_tables(S):
        for r in (1, 3):
            cfg = S.StarkConfig.for_rate(r)
            assert S.prover_memory_plan(stark, cfg, bits, lde="full") == S.prover_memory_plan(stark, cfg, bits, lde=None) > 0, (name, r)


def test_plan_counts_the_words_of_a_small_context_from_below(S):
    """G1Stark 2^9 at rate 3, full: trace, coefficients and LDE of C + Z columns are 10 (C + Z) n words, and the whole plan stays
    within twice that plus the fixed-size buffers (transform scratch of 64 columns, sponge, trees)."""
    stark, cfg = S.G1Stark(), S.StarkConfig.for_rate(3)
    n, m = 512, 4096
    cols = stark.num_columns + stark.num_permutation_zs(cfg)
    plan = S.prover_memory_plan(stark, cfg, 9)
    assert 8 * 10 * cols * n < plan < 8 * (10 * cols * n + (64 + 64) * m * 4)


def test_config4_at_the_recursion_rate_fits_one_card_only_compact(S):
    """Fq12ExpStark(512), for_rate(3), 2^18 rows: values, coefficients and whole LDEs are 10 (C + Z) n words = 359 GB, beyond the 288 GB
    of one MI355X; a compact context keeps 4 (C + Z) n words = 144 GB plus scratch."""
    stark, cfg = S.Fq12ExpStark(512), S.StarkConfig.for_rate(3)
    cols = stark.num_columns + stark.num_permutation_zs(cfg)
    assert cols == 11786 + 5328
    full, compact = S.prover_memory_plan(stark, cfg, 18, lde="full"), S.prover_memory_plan(stark, cfg, 18, lde="compact")
    assert full > 288 * 10**9 and full > 8 * 10 * cols * (1 << 18)
    assert 8 * 4 * cols * (1 << 18) < compact < 160 * 10**9
    assert full - compact == LC.expected_saving(stark, cfg, 18)
