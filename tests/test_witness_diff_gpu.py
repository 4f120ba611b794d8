"""The witness diff on the device (sbn_prover_diff_witness: the device witness written into the coefficient buffer, one compare
pass, one listing pass; csrc/kernels_witdiff.cuh) against the host twin and the numpy reference of tests/witness_diff_cases.py:
report, both per-column arrays and the list, on the smallest trace of each Exp table -- Fq12ExpU64Stark(16) 2^11 rows,
Fq12ExpStark(16) 2^13, G1ExpStark(128), G2ExpStark(128) and FqExpStark(128) 2^16.  Then what must survive the call: the loaded trace,
its public inputs and the proof words, also after a list the generators refuse and on contexts whose shape-constant columns are
resident or whose LDE storage is compact.

Two mutations of the code were tried once each against this file on an MI355X (and withdrawn):
  1. compare_kernel launched without the ragged column tile (grid.y = C / 64, rounded down): caught by
     test_clean_and_single_cells[fq12], [g1] and [g2] -- the tables whose column count is no multiple of 64 (9,802, 1,676, 2,822);
     the single cell in the last column is not seen, cells 0 where the host twin and the reference count 1.  The other ten cases
     run on tables of 9,792 and 960 columns, or change no cell of the last tile, and passed.
  2. wit_select_rows taking rows in descending count order, not in row order: caught by test_caps_and_order (row 70 holds two
     main cells and jumps ahead of row 64), test_main_row_load_with_another_limb and test_given_list_and_changed_exponent.  The
     host twin shares the selection, so it is the numpy reference that catches it -- also without a device, in
     tests/test_witness_diff_host.py::test_host_twin_on_the_u64_table."""
import numpy as np
import pytest

import chained_lists as CL
import tracegen_edges as T
import witness_diff_cases as W

pytestmark = pytest.mark.gpu

TABLES = {"fq12u64": ("fq12expu64_case", "Fq12ExpU64Stark", 11), "fq12": ("fq12exp_case", "Fq12ExpStark", 13), "g1": ("g1exp_case", "G1ExpStark", 16),
          "g2": ("g2exp_case", "G2ExpStark", 16), "fq": ("fqexp_case", "FqExpStark", 16)}
WITNESS = -8


@pytest.fixture(scope="module")
def provers(S):
    """One context per table for the whole module (a G2 context holds several GB), closed at the end."""
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)
    cache = {}

    def get(table):
        if table not in cache:
            _, cls, bits = TABLES[table]
            stark = getattr(S, cls)(16 if table.startswith("fq12") else 128)
            cache[table] = (stark, S.Prover(stark, stark.config(), bits))
        return cache[table]
    yield get
    for _, p in cache.values():
        p.close()


def _same(S, prover, stark, case, loaded, cap=16, ios=None, canonical=None):
    """The loaded trace `loaded`: device == host twin == reference, twice (the second call gives what the first gave)."""
    dev = prover.diff_witness(ios, cap)
    host = S.diff_witness_host(stark, loaded, case["pi"], ios, cap)
    assert dev == host and (cap > 16 or str(dev) == str(host)), (repr(dev), repr(host))
    W.assert_equals_reference(dev, W.reference(loaded, case["trace"] if canonical is None else canonical, stark.num_main_columns, cap))
    assert (dev.pi_words, dev.first_pi_word) == (host.pi_words, host.first_pi_word)
    assert prover.diff_witness(ios, cap) == dev
    times = prover.diff_times()
    assert list(times) == ["witness", "compare", "list_download"] and all(t >= 0 for t in times.values()) and times["witness"] > 0
    return dev


@pytest.mark.parametrize("table", list(TABLES))
def test_clean_and_single_cells(S, provers, request, table):
    """(a) the oracle's trace is the canonical witness: zero everywhere.  (b) one cell alone: on the smallest table each of (0, 0),
    (n - 1, num_main - 1), (63, 63), (64, 64), (n - 1, C - 1); on G1 the cell in the last, ragged tile column 1,675; on the other
    tables the last cell."""
    case = request.getfixturevalue(TABLES[table][0])
    stark, prover = provers(table)
    n, num_main, Cn = case["trace"].shape[1], stark.num_main_columns, stark.num_columns
    prover.load_trace(case["trace"], case["pi"])
    dev = _same(S, prover, stark, case, case["trace"])
    assert dev.ok and dev.cells == 0 and dev.listed == [] and dev.first_row is None and not dev.column_cells.any()
    assert (dev.column_first_row == W.NO_ROW).all()
    cells = W.single_cells(n, num_main, Cn) if table == "fq12u64" else [(100, Cn - 1)]
    assert table != "g1" or cells == [(100, 1675)]
    for cell in cells:
        bad = W.plant(case["trace"], [cell])
        prover.load_trace(bad, case["pi"])
        dev = _same(S, prover, stark, case, bad)
        assert (dev.cells, dev.rows, dev.columns, dev.first_row, dev.first_column) == (1, 1, 1) + cell and not dev.ok
        assert dev.listed[0]["instance"] == cell[0] // dev.rows_per_instance and dev.listed[0]["checked_by"]
    assert np.array_equal(prover.read_trace(), bad)


def test_whole_column(S, provers, fq12expu64_case):
    """(c) every cell of one main column: the counts stay exact under a cap of 16, the list is the first 16 of the reference."""
    stark, prover = provers("fq12u64")
    bad = W.plant(fq12expu64_case["trace"], W.whole_column(2048, 7))
    prover.load_trace(bad, fq12expu64_case["pi"])
    dev = _same(S, prover, stark, fq12expu64_case, bad)
    assert (dev.cells, dev.main_cells, dev.rows, dev.columns, len(dev.listed)) == (2048, 2048, 2048, 1, 16)
    assert [q["row"] for q in dev.listed] == list(range(16))


def test_whole_row(S, provers, fq12expu64_case):
    """(c) every cell of one row, 9,792 of them: the cap of 16 cuts inside the row."""
    stark, prover = provers("fq12u64")
    bad = W.plant(fq12expu64_case["trace"], W.whole_row(stark.num_columns, 129))
    prover.load_trace(bad, fq12expu64_case["pi"])
    dev = _same(S, prover, stark, fq12expu64_case, bad)
    assert (dev.cells, dev.main_cells, dev.rows, dev.columns) == (stark.num_columns, stark.num_main_columns, 1, stark.num_columns)
    assert [q["column"] for q in dev.listed] == list(range(16))
    everything = _same(S, prover, stark, fq12expu64_case, bad, cap=stark.num_columns)      # the main columns, then the derived ones
    assert [q["column"] for q in everything.listed] == list(range(stark.num_columns))


def test_caps_and_order(S, provers, fq12expu64_case):
    """(d) caps 0, 1, cells and cells + 5 over seven scattered cells: four main ones on three rows, three derived ones of which one
    lies on an earlier row than any main cell."""
    stark, prover = provers("fq12u64")
    cells = W.scattered(2048, stark.num_main_columns, stark.num_columns)
    bad = W.plant(fq12expu64_case["trace"], cells)
    prover.load_trace(bad, fq12expu64_case["pi"])
    for cap in (0, 1, len(cells), len(cells) + 5):
        dev = _same(S, prover, stark, fq12expu64_case, bad, cap)
        assert len(dev.listed) == min(cap, len(cells)) and (dev.cells, dev.main_cells) == (7, 4)
        assert (dev.first_row, dev.first_column) == (64, 64)
    assert [q["row"] for q in dev.listed] == [64, 70, 70, 2047, 5, 200, 2046]
    for cap in (65537, -1):
        with pytest.raises(S.SbnError) as e:
            prover.diff_witness(None, cap)
        assert e.value.code == -1


def test_list_in_several_launches(S, provers, fq12expu64_case):
    """20 whole main columns = 40,960 cells under the largest cap: 1.3 MB of cells against the 1 MiB of scratch a 2^11-row context
    has, so the listing takes more than one launch."""
    stark, prover = provers("fq12u64")
    bad = W.plant(fq12expu64_case["trace"], [cell for c in range(20) for cell in W.whole_column(2048, 3 * c)])
    prover.load_trace(bad, fq12expu64_case["pi"])
    dev = _same(S, prover, stark, fq12expu64_case, bad, cap=65536)
    assert (dev.cells, dev.rows, dev.columns, len(dev.raw_cells)) == (40960, 2048, 20, 40960)


def test_main_row_load_with_another_limb(S, provers, g1exp_case):
    """(e) G1 loaded through load_trace_rows in main-row mode with one u16 limb replaced by another u16 value (bit 15 flipped, on
    row 65,000): one main cell; the sorted range-check columns the device derives moved as a consequence, between the sorted
    positions of the two values and so on EARLIER rows; the list still opens with the main cell."""
    stark, prover = provers("g1")
    num_main = stark.num_main_columns
    rows = np.ascontiguousarray(g1exp_case["trace"][:num_main].T)
    row, col = 65000, 64 + 16                                          # new_x limb 0 of the add gadget: range-checked
    assert int(rows[row, col]) < 1 << 16
    rows[row, col] = int(rows[row, col]) ^ 0x8000
    prover.load_trace_rows(rows, g1exp_case["pi"])
    loaded = prover.read_trace()
    assert np.array_equal(loaded[:num_main], rows.T)
    dev = _same(S, prover, stark, g1exp_case, loaded)
    assert dev.main_cells == 1 and dev.cells > 1 and (dev.first_row, dev.first_column) == (row, col)
    assert (dev.listed[0]["row"], dev.listed[0]["column"], dev.listed[0]["main"]) == (row, col, True) and not dev.listed[1]["main"]
    derived = dev.column_cells[num_main:] > 0
    assert derived.any() and int(dev.column_first_row[num_main:][derived].min()) < row


def test_given_list_and_changed_exponent(S, provers, fq12expu64_case):
    """(f) ios=None and ios=case["ios"] agree; an ios with one changed exponent bit gives pi_words > 0 and the diff against THAT
    list's host trace."""
    stark, prover = provers("fq12u64")
    c = fq12expu64_case
    bad = W.plant(c["trace"], [(300, 5), (301, 9000)])
    prover.load_trace(bad, c["pi"])
    assert _same(S, prover, stark, c, bad) == _same(S, prover, stark, c, bad, ios=c["ios"])
    ios = np.array(c["ios"], dtype=np.uint32)
    ios[3, 192] ^= 2
    other, other_pi = stark.generate_trace_and_public_inputs(ios)
    prover.load_trace(c["trace"], c["pi"])
    dev = _same(S, prover, stark, c, c["trace"], 16, ios, other)
    assert dev.cells > 0 and dev.pi_words == int((other_pi != c["pi"]).sum()) > 0
    assert dev.first_pi_word == int(np.nonzero(other_pi != c["pi"])[0][0]) and dev.listed[0]["instance"] == 3


def test_refused_list_leaves_the_trace_loaded(S, provers, g1exp_case):
    """(g) a list the generators refuse (chained_lists.witness_refusals, 'collide': the table's first addition meets B = A) returns
    SBN_ERR_WITNESS behind the prefix; the caller's trace is still loaded and prove() gives the words it gave before.  (h) the
    same on this full context once its shape-constant columns are resident: a diff that ran leaves the proof words alone."""
    stark, prover = provers("g1")
    prover.load_trace(g1exp_case["trace"], g1exp_case["pi"])
    before = prover.prove().words
    assert np.array_equal(prover.prove().words, before)
    assert int(prover.describe()["fixed_columns_skipped"]) > 0       # the transforms of the shape-constant columns are resident
    xs, es, start = CL.witness_refusals("g1")["collide"]
    refused = T.pack("g1", CL.derive("g1", xs, es, start)[0])
    with pytest.raises(S.SbnError) as e:
        prover.diff_witness(refused)
    assert e.value.code == WITNESS and "no canonical witness: " in str(e.value)
    assert np.array_equal(prover.prove().words, before)
    assert np.array_equal(prover.read_trace(), g1exp_case["trace"])
    assert prover.diff_witness().ok
    assert np.array_equal(prover.prove().words, before)
    assert np.array_equal(prover.prove().words, before)              # ... and once more with the columns resident again
    assert prover.diff_witness(g1exp_case["ios"], 0).ok


def test_prove_on_a_compact_rate3_context(S, fq12expu64_case):
    """(h) a compact rate-3 Fq12ExpU64Stark(16) context: the scratch of the generators is carved from the thinned LDE buffer."""
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    S.lib().sbn_set_device(0)
    stark, c = S.Fq12ExpU64Stark(16), fq12expu64_case
    prover = S.Prover(stark, S.StarkConfig.for_rate(3), 11, lde="compact")
    with pytest.raises(S.SbnError) as e:
        prover.diff_witness()
    assert e.value.code == -1 and "no trace loaded" in str(e.value)
    bad = W.plant(c["trace"], [(0, 0), (2047, stark.num_columns - 1)])
    prover.load_trace(bad, c["pi"])
    before = prover.prove().words
    dev = prover.diff_witness()
    W.assert_equals_reference(dev, W.reference(bad, c["trace"], stark.num_main_columns, 16))
    assert dev == S.diff_witness_host(stark, bad, c["pi"])
    assert np.array_equal(prover.prove().words, before) and np.array_equal(prover.read_trace(), bad)
    prover.close()
