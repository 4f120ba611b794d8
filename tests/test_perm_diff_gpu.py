"""The values and rows behind a failing permutation pair on the device (sbn_prover_explain_permutations: signed histograms in LDS,
csrc/kernels_permdiff.cuh) against the host form and the numpy reference of tests/perm_diff_cases.py, entry for entry: a height
below a workgroup's stride, all 65,536 bins in use, rows and counts above 2^16, and the three routes of cells that no bin takes."""
import numpy as np
import pytest

import check_trace_cases as K
import perm_diff_cases as PC

pytestmark = pytest.mark.gpu


def _device(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)


def _routes(prover):
    """Pairs of the last explain_permutations() answered by the bins alone, with the overflow list, from downloaded columns."""
    return tuple(int(x) for x in prover.describe()["perm_diff_routes"].split(":"))


def _same(S, prover, stark, bad, clean=None, changed=(), zs=None, per_pair=8):
    """The loaded trace `bad`: device == host == reference; returns the device result."""
    dev = prover.explain_permutations(zs, per_pair)
    host = S.explain_permutations_host(stark, bad, zs, per_pair)
    assert dev == host and str(dev) == str(host)
    assert np.array_equal(dev.stats, host.stats)
    PC.assert_equals_reference(dev, PC.reference(stark, bad, zs, per_pair, clean=clean, changed=changed))
    times = prover.explain_permutation_times()
    assert list(times) == ["histogram", "rows", "download_merge"] and all(t >= 0 for t in times.values())
    assert sum(_routes(prover)) == len(dev.zs)
    return dev


def _seam_cells(c, k=1):
    """The six values of PC.SEAM_VALUES in six rows of the rhs column of a pair in the middle of the table."""
    Z = c["stark"].num_permutation_zs()
    z = (Z // 2 + k) % Z
    rhs = c["stark"].permutation_pair(z)[1]
    return z, [(rhs, row, v) for row, v in zip([3, 100, 255, 256, 300, c["n"] - 1], PC.SEAM_VALUES)]


def test_g1op_512_rows(S):
    """n below the stride of a workgroup; 1,264 pairs, which the 256 KiB of scratch at this height takes in several launches."""
    _device(S)
    c = K.case("g1op")
    stark = c["stark"]
    prover = S.Prover(stark, stark.config(), 9)
    with pytest.raises(S.SbnError) as e:
        prover.explain_permutations()
    assert e.value.code == -1                                        # no trace loaded
    prover.load_trace(c["trace"], c["pi"])
    assert _same(S, prover, stark, c["trace"], c["trace"]).ok
    assert _routes(prover) == (stark.num_permutation_zs(), 0, 0)
    z, cells = _seam_cells(c)
    for cell in cells[:4] + [(cells[0][0], 0, PC.other_value(c["trace"], cells[0][0], 0)), (cells[0][0], 511, PC.other_value(c["trace"], cells[0][0], 511))]:
        bad, changed = PC.set_cells(c["trace"], [cell])
        prover.load_trace(bad, c["pi"])
        assert not _same(S, prover, stark, bad, c["trace"], changed).ok
        assert _routes(prover)[1:] == (0, 0)
    for cell in cells[4:]:                                           # 65536 and p - 1: the overflow list
        bad, changed = PC.set_cells(c["trace"], [cell])
        prover.load_trace(bad, c["pi"])
        _same(S, prover, stark, bad, c["trace"], changed)
        assert _routes(prover)[1] >= 1 and _routes(prover)[2] == 0
    bad, changed = PC.set_cells(c["trace"], cells)
    prover.load_trace(bad, c["pi"])
    dev = _same(S, prover, stark, bad, c["trace"], changed, per_pair=16)
    assert [e["value"] for q in dev.pairs if q["z"] == z for e in q["entries"]][-2:] == [65536, PC.P - 1]
    _same(S, prover, stark, bad, c["trace"], changed, per_pair=3)    # the cap cuts inside the binned values
    _same(S, prover, stark, bad, c["trace"], changed, per_pair=0)
    _same(S, prover, stark, bad, c["trace"], changed, zs=[z, 0, z + 1], per_pair=2000)
    with pytest.raises(S.SbnError) as e:
        prover.explain_permutations(zs=[stark.num_permutation_zs()])
    assert e.value.code == -1
    assert np.array_equal(prover.read_trace(), bad)
    prover.close()


def test_g1exp_all_bins_in_use(S):
    """2^16 rows, u16 pairs: every one of the 65,536 bins holds a count.  The seam and end cells, the two values no bin takes, then
    one cell of EVERY rhs column changed at once: every pair fails, every workgroup of the rows pass works."""
    _device(S)
    c = K.case("g1exp")
    stark, n, Z = c["stark"], c["n"], c["stark"].num_permutation_zs()
    prover = S.Prover(stark, stark.config(), 16)
    prover.load_trace(c["trace"], c["pi"])
    assert _same(S, prover, stark, c["trace"], c["trace"]).ok
    assert _routes(prover) == (Z, 0, 0)
    z, cells = _seam_cells(c)
    bad, changed = PC.set_cells(c["trace"], cells)
    prover.load_trace(bad, c["pi"])
    dev = _same(S, prover, stark, bad, c["trace"], changed, per_pair=16)
    assert not dev.ok and _routes(prover)[1] >= 1 and _routes(prover)[2] == 0
    rhs_cols = sorted({stark.permutation_pair(z)[1] for z in range(Z)})
    every = [(col, (37 * k) % n, PC.other_value(c["trace"], col, (37 * k) % n)) for k, col in enumerate(rhs_cols)]
    bad, changed = PC.set_cells(c["trace"], every)
    prover.load_trace(bad, c["pi"])
    dev = _same(S, prover, stark, bad, c["trace"], changed)
    assert len(dev.pairs) == Z and all(q["differing_values"] == 2 or q["lhs_col"] in changed for q in dev.pairs)
    prover.close()


def test_rows_and_counts_above_2_16(S):
    """ModularStark's 8,192-row trace tiled to 2^17 rows: row indices above 2^16, and the value 255 on both sides of the table
    pairs far more often than a 16-bit counter holds."""
    _device(S)
    c = K.case("modular_8192")
    stark = c["stark"]
    trace = np.tile(c["trace"], 16)
    n = trace.shape[1]
    assert n == 1 << 17
    prover = S.Prover(stark, stark.config(), 17)
    prover.load_trace(trace, c["pi"])
    assert _same(S, prover, stark, trace).ok
    z, rhs = [(z, r) for z in range(stark.num_permutation_zs()) for r in [stark.permutation_pair(z)[1]] if np.count_nonzero(trace[r] == 255) > 65535][0]
    row = int(np.nonzero(trace[rhs] == 255)[0][-1])
    assert row > 1 << 16
    bad, _ = PC.set_cells(trace, [(rhs, row, 254)])
    prover.load_trace(bad, c["pi"])
    dev = _same(S, prover, stark, bad)
    q = [q for q in dev.pairs if q["z"] == z][0]
    e = [e for e in q["entries"] if e["value"] == 255][0]
    assert e["count_lhs"] > 65535 and e["count_rhs"] == e["count_lhs"] - 1
    prover.close()


@pytest.mark.parametrize("bits, route", [(9, 1), (17, 2)])
def test_lookup_values_no_bin_takes(S, bits, route):
    """A 4-column LookupStark matrix of random 64-bit words: at 512 rows the overflow list holds every cell (route 1), at 2^17 rows
    4 * 2^17 cells overflow it and both pairs are downloaded (route 2).  Clean, then three cells changed."""
    _device(S)
    stark = S.MyStark()
    n = 1 << bits
    m = PC.lookup_matrix(n, 11 + bits)
    prover = S.Prover(stark, stark.config(), bits)
    prover.load_trace(m, K.NOPI)
    assert _same(S, prover, stark, m).ok
    expect = tuple(2 if r == route else 0 for r in range(3))
    assert _routes(prover) == expect
    bad, _ = PC.set_cells(m, [(2, 0, 5), (2, n - 1, PC.P - 1), (3, n // 2 + 1, int(m[3, 4]))])
    prover.load_trace(bad, K.NOPI)
    dev = _same(S, prover, stark, bad)
    assert [q["z"] for q in dev.pairs] == [0, 1] and _routes(prover) == expect
    assert dev.pairs[0]["entries"][0] == {"value": 5, "count_lhs": 0, "count_rhs": 1, "first_row_lhs": None, "first_row_rhs": 0}
    prover.close()


def test_prove_gives_the_same_words_before_and_after(S):
    """Only per-proof scratch is overwritten: Fq12ExpStark, 512 rows, a valid trace."""
    _device(S)
    c = K.case("fq12exp")
    prover = S.Prover(c["stark"], c["stark"].config(), 9)
    prover.load_trace(c["trace"], c["pi"])
    before = prover.prove().words
    assert _same(S, prover, c["stark"], c["trace"], c["trace"]).ok
    assert np.array_equal(prover.prove().words, before)
    assert np.array_equal(prover.read_trace(), c["trace"])
    prover.close()
