"""The shape-constant trace columns (include/sbn.h sbn_fixed_columns_range), without a GPU: the range the prover keeps transformed
between proofs is exactly the block the host witness generators fill without reading the instance list -- same words for two
instance lists, closed forms where they are cheap to restate, witness columns right outside it -- and empty for the tables that
have no such block."""
import numpy as np
import pytest

# (table class, conftest case of list A, oracle input generator and seed of list B, rows per instance, has a periodic pulse)
EXP_TABLES = {
    "g1exp": ("G1ExpStark", "g1exp_case", "g1exp_inputs", 128, 101, 512, True),
    "g2exp": ("G2ExpStark", "g2exp_case", "g2exp_inputs", 128, 102, 512, True),
    "fq12exp": ("Fq12ExpStark", "fq12exp_case", "fq12exp_inputs", 16, 103, 512, True),
    "fqexp": ("FqExpStark", "fqexp_case", "fqexp_inputs", 128, 104, 512, True),
    "fq12expu64": ("Fq12ExpU64Stark", "fq12expu64_case", "fq12expu64_inputs", 16, 105, 128, False),
}


@pytest.mark.parametrize("table", sorted(EXP_TABLES))
def test_range_is_the_block_the_generator_fills_without_the_instances(table, S, O, request):
    cls, case, inputs, num_io, seed_b, rpb, periodic = EXP_TABLES[table]
    stark = getattr(S, cls)(num_io)
    f0, f1 = S.api.fixed_columns_range(stark)
    assert f1 - f0 == (2 if periodic else 0) + 1 + 4 * num_io + 1 and 0 < f0 and f1 < stark.num_columns
    a = request.getfixturevalue(case)["trace"]                       # list A: the suite's seeded trace of this table
    ios_b, _ = getattr(O, inputs)(num_io, seed_b)                    # list B: other instances, the product's host generator
    b = stark.generate_trace(ios_b)
    assert a.shape == b.shape and not np.array_equal(a[:f0], b[:f0])
    assert np.array_equal(a[f0:f1], b[f0:f1])
    # the block is what the reference's pulse and lookup generators write: counters, pulses at the first and last row of every
    # instance, the table column
    n = a.shape[1]
    rows = np.arange(n, dtype=np.uint64)
    io0 = f0 + (2 if periodic else 0)
    if periodic:
        assert np.array_equal(b[f0], (rows + 1) % 64)
    assert np.array_equal(b[io0], rows)
    for q in (0, 1, 2 * num_io - 1):
        pos = (q // 2) * rpb + (rpb - 1 if q % 2 else 0)
        pulse = np.zeros(n, dtype=np.uint64)
        pulse[pos] = 1
        assert np.array_equal(b[io0 + 2 + 2 * q], pulse) and int(b[io0 + 1 + 2 * q, pos]) == 0
    assert int(b[f1 - 1, 0]) == 0 and int(b[f1 - 1, 255]) == 255 and np.array_equal(b[f1 - 1], np.minimum(rows, b[f1 - 1, -1]))
    if table == "g1exp":
        assert (f0, f1) == (398, 914)
        # right outside either end: the last exponent limb of the flags block, the first sorted range-check column
        assert not np.array_equal(a[f0 - 1], b[f0 - 1]) and not np.array_equal(a[f1], b[f1])


def test_range_is_empty_for_the_other_tables(S):
    others = [S.G1Stark(), S.ModularStark(), S.Fq12Stark(), S.LookupStark(), S.FlagStark(16), S.FlagU64Stark(16)]
    assert len({type(t) for t in others}) == 6
    for stark in others:
        assert S.api.fixed_columns_range(stark) == (0, 0)


def test_switch_is_a_checked_setting(S, monkeypatch):
    """SBN_FIXED_COLUMNS is read with the other switches (every settings check and every prover creation reads the environment
    anew): 0 or 1, anything else is refused."""
    for value, ok in (("0", True), ("1", True), ("2", False), ("on", False)):
        monkeypatch.setenv("SBN_FIXED_COLUMNS", value)
        if ok:
            S.api.settings_check()
        else:
            with pytest.raises(S.SbnError) as e:
                S.api.settings_check()
            assert e.value.code == -1 and "SBN_FIXED_COLUMNS" in str(e.value)
