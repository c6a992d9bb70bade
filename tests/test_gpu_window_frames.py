"""Sliding window frames on the GPU.  At the C ABI (hs_window_frames) INTEGER results and FLOAT results
over small whole numbers must be EXACTLY those of the model (tests/window_frame_model.py), a FLOAT sum of general values
is held to test_gpu_window_agg's bound of an f64 sum under any association, FIRST_VALUE / LAST_VALUE are compared bit for
bit, and a NaN or an infinity must show in exactly the rows whose frame holds it.  End to end: queries over the committed
golden tables through engine.sql and the DataFrame API against the model applied to the rows the same engine returns for
the query without its window items."""

from __future__ import annotations

import json
import math

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, load_golden
from tests.ranks import run_ranks
from tests.test_gpu_distinct import py_values, tuples, upload
from tests.test_gpu_window import FLOATS, OB_TILE, ROW_NUMBER, hs_window
from tests.test_gpu_window_agg import AVG, COUNT, FLT_OVERFLOW, INT_OVERFLOW, MAX, MIN, SUM, avg32, f32, hs_window_agg, ulp32
from tests.test_gpu_window_nav import FIRST_VALUE, LAG, LAST_VALUE, LEAD, NTILE, cells_of, hs_window_nav, untouched
from tests.window_abi import call_window
from tests.window_frame_model import window_frame_exact, window_frame_model

pytestmark = pytest.mark.gpu

K_MAX = (1 << 31) - 1
ROWS = [1, 2, OB_TILE - 1, OB_TILE, OB_TILE + 1, 3 * OB_TILE + 5]
# CURRENT ROW alone; one neighbour on either side; both sides; a block of one tile less a row / one tile more a row; W = 1024,
# a block head on every tile boundary; a frame wider than two tiles, blocks that straddle several
PAIRS = [(0, 0), (1, 0), (0, 1), (3, 2), (OB_TILE - 1, 0), (0, OB_TILE), (1000, 23), (5000, 5000)]


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def hs_window_frames(dev, cols, descending, n_part, items, n, n_keys=None, no_preceding=False, no_following=False):
    """The entry point itself.  items = [(function, frame name or code, value column or None, n PRECEDING, m FOLLOWING[, k,
    default bits])] -> (return code, [one array per item, input order: the cells' bits as uint32, uint64 for an 8-byte
    argument], the status word).  Every output has a sentinel in SLACK cells behind the rows, which must stay untouched."""
    omit = [name for name, off in (("preceding", no_preceding), ("following", no_following)) if off]
    behind = [(*it[:3], *it[5:7], *[None] * (2 - len(it[5:7])), *it[3:5]) for it in items]  # the harness: k, default, then n, m
    return call_window(dev, "hs_window_frames", cols, descending, n_part, behind, n, n_keys, omit)


def said(dev):
    return dev._raw_lib.hs_last_error()


def partitionings(n, rng):
    """(name, partition id per SORTED place)"""
    place = np.arange(n)
    out = [("one partition", np.zeros(n, dtype=np.int64)), ("partitions of 1 row", place.copy()),
           ("random partitions of 1 - 40 rows", np.repeat(np.arange(n), rng.integers(1, 41, n))[:n])]
    if n > OB_TILE:
        out.append(("a partition starts at a tile's first row", (place >= OB_TILE).astype(np.int64)))
    return out


def keyed(dev, rng, ids):
    """PARTITION BY an INTEGER, ORDER BY an INTEGER that two neighbouring places share (ties: input order decides), the rows
    shuffled -> (uploaded key columns, the model's partition, the model's order, the shuffle)"""
    n = len(ids)
    shuffle = rng.permutation(n)
    part, order = (ids * 7 - 3)[shuffle], (np.arange(n) // 2 - 50)[shuffle]
    cols = [upload(dev, part, T.INTEGER), upload(dev, order, T.INTEGER)]
    return cols, [py_values(part, T.INTEGER)], [(py_values(order, T.INTEGER), True)], shuffle


def differs(column, expected, where):
    bad = np.nonzero(column != expected)[0]
    assert bad.size == 0, (f"{where}: differs at {bad.size} of {column.size} rows, first row {bad[0]}: got {column[bad[0]]!r}, "
                           f"want {expected[bad[0]]!r}")


@pytest.mark.parametrize("n", ROWS)
def test_integer_and_whole_float_aggregates_are_exactly_the_model(dev, n):
    """Cells are whole numbers below 2^16 in size: no sum leaves i32, and as f32 every f64 partial sum of them is exact, so
    the FLOAT results do not depend on the association and are the INTEGER ones rounded once."""
    rng = np.random.default_rng(n)
    for name, ids in partitionings(n, rng):
        cols, part, order, _ = keyed(dev, rng, ids)
        cells = rng.integers(-50000, 50001, n)
        whole, real = upload(dev, cells, T.INTEGER), upload(dev, cells.astype(np.float32), T.FLOAT)
        for pre, fol in PAIRS:
            want = window_frame_exact(n, part, order, py_values(cells, T.INTEGER), pre, fol)
            count, total = np.asarray(want["count"], dtype=np.int64), np.asarray(want["sum"], dtype=np.int64)
            low, high = np.asarray(want["min"], dtype=np.int64), np.asarray(want["max"], dtype=np.int64)
            rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, [(f, "between", whole, pre, fol) for f in (COUNT, SUM, MIN, MAX, AVG)], n)
            assert rc == 0 and flags == 0, (said(dev), flags)
            where = f"{name}, ({pre}, {fol})"
            for column, expected, f in zip(got[:4], (count, total, low, high), "count sum min max".split()):
                differs(column.view(np.int32), expected, f"{where}, INTEGER {f}")
            differs(got[4].view(np.float32), avg32(total, count), f"{where}, INTEGER avg")
            items = [(f, "between", real, pre, fol) for f in (SUM, MIN, MAX, AVG)]
            items += [(FIRST_VALUE, "between", whole, pre, fol), (LAST_VALUE, "between", whole, pre, fol)]
            rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, items, n)
            assert rc == 0 and flags == 0, (said(dev), flags)
            for column, expected, f in zip(got[:4], (f32(total), f32(low), f32(high), avg32(total, count)), "sum min max avg".split()):
                differs(column.view(np.float32), expected, f"{where}, FLOAT {f}")
            differs(got[4].view(np.int32), cells[np.asarray(want["first"])], f"{where}, first_value")
            differs(got[5].view(np.int32), cells[np.asarray(want["last"])], f"{where}, last_value")


def test_the_fast_model_is_the_brute_force_at_a_tile_boundary():
    """what the test above compares with, held against the definition's own walk on one of its shapes"""
    n, rng = OB_TILE + 1, np.random.default_rng(5)
    ids = np.repeat(np.arange(n), rng.integers(1, 41, n))[:n]
    order, cells = (np.arange(n) // 2).tolist(), rng.integers(-50000, 50001, n).tolist()
    for pre, fol in ((3, 2), (0, 40), (25, 25)):
        assert window_frame_exact(n, [ids.tolist()], [(order, True)], cells, pre, fol) == \
            window_frame_model(n, [ids.tolist()], [(order, True)], cells, pre, fol)


@pytest.mark.parametrize("n", ROWS)
def test_a_frame_of_the_widest_offsets_is_the_partition_frame_bit_for_bit(dev, n):
    """(2^31 - 1, 2^31 - 1): W = 2^32 - 1 needs 64 bits, and every frame is the row's partition."""
    rng = np.random.default_rng(11 * n)
    for name, ids in partitionings(n, rng):
        cols, _, _, _ = keyed(dev, rng, ids)
        whole = upload(dev, rng.integers(-50000, 50001, n), T.INTEGER)
        funcs = (SUM, AVG, MIN, MAX, COUNT, FIRST_VALUE, LAST_VALUE)
        rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, [(f, "between", whole, K_MAX, K_MAX) for f in funcs], n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        rc, want, flags = hs_window_nav(dev, cols, [0, 0], 1, [(f, "partition", whole) for f in funcs], n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        for f, mine, theirs in zip(funcs, got, want):
            differs(mine, theirs, f"{name}, function {f}")


def numpy_frames(ids, cells, pre, fol):
    """INTEGER cells by SORTED place -> (count, sum, min, max) per place, vectorised: the frame's ends from the definition,
    sums as differences of an int64 prefix (whole numbers: exact), MIN / MAX from a sparse table."""
    n = len(ids)
    place = np.arange(n, dtype=np.int64)
    head = np.append(True, ids[1:] != ids[:-1])
    first = np.maximum.accumulate(np.where(head, place, 0))
    last = np.minimum.accumulate(np.where(np.append(head[1:], True), place, n)[::-1])[::-1]
    lo, hi = np.maximum(first, place - pre), np.minimum(last, place + fol)
    prefix = np.append(0, np.cumsum(cells.astype(np.int64)))
    count = hi - lo + 1
    level = np.floor(np.log2(count)).astype(np.int64)
    least, greatest = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    low = high = cells.astype(np.int64)
    for k in range(int(level.max()) + 1):
        if k:
            half = 1 << (k - 1)
            low, high = np.minimum(low[:-half], low[half:]), np.maximum(high[:-half], high[half:])
        at = np.nonzero(level == k)[0]
        least[at] = np.minimum(low[lo[at]], low[hi[at] + 1 - (1 << k)])
        greatest[at] = np.maximum(high[lo[at]], high[hi[at] + 1 - (1 << k)])
    return count, prefix[hi + 1] - prefix[lo], least, greatest


def test_frames_across_a_round_of_the_tile_scan(dev):
    """The tile-carry kernel takes OB_TILE summaries per round: rows beyond OB_TILE tiles lie in its second round.  Three
    partitions in order, the middle one starting 1500 places before the round's boundary and ending 700 behind it; frames of
    (3000, 3000) reach across the boundary from both sides, forward and backward carry alike.  INTEGER cells, exact."""
    n, edge = OB_TILE * OB_TILE + OB_TILE + 1, OB_TILE * OB_TILE
    rng = np.random.default_rng(23)
    place = np.arange(n)
    ids = np.where(place < edge - 1500, 0, np.where(place < edge + 700, 1, 2))
    cells = rng.integers(-300, 301, n)
    small = slice(0, 3000)  # the vectorised expectation against the model on a prefix with its own partitions
    check = numpy_frames(place[small] // 700, cells[small], 300, 200)
    model = window_frame_exact(3000, [(place[small] // 700).tolist()], [], cells[small].tolist(), 300, 200)
    assert all(np.array_equal(a, np.asarray(model[k])) for a, k in zip(check, ("count", "sum", "min", "max")))
    cols = [upload(dev, ids, T.INTEGER), upload(dev, place, T.INTEGER)]
    value = upload(dev, cells, T.INTEGER)
    for pre, fol in ((3000, 3000), (1, 0)):
        rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, [(f, "between", value, pre, fol) for f in (COUNT, SUM, MIN, MAX)], n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        for column, expected, f in zip(got, numpy_frames(ids, cells, pre, fol), "count sum min max".split()):
            differs(column.view(np.int32), expected, f"({pre}, {fol}), {f}")


@pytest.mark.parametrize("n", ROWS[-2:])
def test_float_sums_of_general_values_stay_inside_the_f64_bound(dev, n):
    """test_gpu_window_agg's bound, row by row: |got - X| <= (m - 1) 2^-52 sum|x| + ulp_f32(max(|got|, |X|)) / 2 with X the
    exact frame sum and m its rows - an f64 sum of m terms under ANY association, then one rounding to f32; AVG the same
    divided by m plus its own half ulp.  And the same call twice gives the same bits."""
    rng = np.random.default_rng(3 * n)
    for name, ids in partitionings(n, rng):
        cols, part, order, _ = keyed(dev, rng, ids)
        cells = (rng.uniform(-1e6, 1e6, n) * 2.0 ** rng.integers(-30, 1, n)).astype(np.float32)
        value = upload(dev, cells, T.FLOAT)
        pairs = [(3, 2), (0, OB_TILE), (5000, 5000), (1000, 23)]
        items = [(f, "between", value, pre, fol) for pre, fol in pairs for f in (SUM, AVG)]
        rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        rc, again, _ = hs_window_frames(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, again))
        for k, (pre, fol) in enumerate(pairs):
            want = window_frame_exact(n, part, order, py_values(cells, T.FLOAT), pre, fol)
            X, m, mass = np.asarray(want["sum"]), np.asarray(want["count"], dtype=np.float64), np.asarray(want["abs"])
            s, a = got[2 * k].view(np.float32).astype(np.float64), got[2 * k + 1].view(np.float32).astype(np.float64)
            bound = (m - 1) * 2.0 ** -52 * mass + 0.5 * ulp32(np.maximum(np.abs(s), np.abs(X)))
            off = np.abs(s - X)
            print(f"n={n} {name} ({pre}, {fol}): SUM worst |got - X| / bound = {np.max(off / bound):.3g}")
            assert np.all(off <= bound), (name, pre, fol, int(np.argmax(off - bound)))
            bound_avg = bound / m + 0.5 * ulp32(np.maximum(np.abs(a), np.abs(X / m)))
            off = np.abs(a - X / m)
            print(f"n={n} {name} ({pre}, {fol}): AVG worst |got - X/m| / bound = {np.max(off / bound_avg):.3g}")
            assert np.all(off <= bound_avg), (name, pre, fol, int(np.argmax(off - bound_avg)))


def test_a_nan_and_the_infinities_show_in_exactly_the_rows_whose_frame_holds_them(dev):
    """What a difference of two running sums fails: the row just behind the last frame that holds the NaN is finite again.
    Partition 1 lies across a tile boundary and is all NaN / inf / -inf / 2.5: nothing of it shows in its neighbours."""
    n = OB_TILE + 100
    place = np.arange(n)
    ids = np.where(place < OB_TILE - 10, 0, np.where(place < OB_TILE + 10, 1, 2))
    rng = np.random.default_rng(8)
    cells = (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32)  # every f64 partial sum is exact
    middle = np.nonzero(ids == 1)[0]
    cells[middle] = np.resize(np.array([np.nan, np.inf, 2.5, -np.inf], dtype=np.float32), middle.size)
    at_nan, at_pinf, at_ninf = 500, 900, 1300  # in partition 0, far from one another
    cells[at_nan], cells[at_pinf], cells[at_ninf] = np.nan, np.inf, -np.inf
    shuffle = rng.permutation(n)
    where = np.empty(n, dtype=np.int64)
    where[shuffle] = place  # where[p]: the row that stands at sorted place p
    cols = [upload(dev, ids[shuffle], T.INTEGER), upload(dev, place[shuffle], T.INTEGER)]
    value = upload(dev, cells[shuffle], T.FLOAT)
    part, order = [py_values(ids[shuffle], T.INTEGER)], [(py_values(place[shuffle], T.INTEGER), True)]
    for pre, fol in ((3, 2), (0, 4), (40, 0)):
        rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, [(f, "between", value, pre, fol) for f in (SUM, MIN, MAX, AVG)], n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        got = [column.view(np.float32) for column in got]
        want = window_frame_model(n, part, order, py_values(cells[shuffle], T.FLOAT), pre, fol)
        for column, k in zip(got[:3], ("sum", "min", "max")):  # NaN where the model has one, else its value
            expected = f32(want[k])
            assert np.array_equal(np.isnan(column), np.isnan(expected)), (pre, fol, k)
            assert np.array_equal(column[~np.isnan(expected)], expected[~np.isnan(expected)]), (pre, fol, k)
        by_place = got[0][where]  # SUM by sorted place
        # place j holds the NaN in its frame iff j - pre <= at_nan <= j + fol
        assert np.all(np.isnan(by_place[at_nan - fol:at_nan + pre + 1]))
        assert np.isfinite(by_place[at_nan - fol - 1]) and np.isfinite(by_place[at_nan + pre + 1])
        assert np.all(by_place[at_pinf - fol:at_pinf + pre + 1] == np.inf) and np.isfinite(by_place[at_pinf + pre + 1])
        assert np.all(by_place[at_ninf - fol:at_ninf + pre + 1] == -np.inf) and np.isfinite(by_place[at_ninf - fol - 1])
        outside = np.ones(n, dtype=bool)
        for at in (at_nan, at_pinf, at_ninf):
            outside[max(0, at - fol):at + pre + 1] = False
        outside[middle] = False
        assert np.all(np.isfinite(by_place[outside])) and np.all(np.isfinite(got[3][where][outside]))  # the neighbours of partition 1 too
        # the NaN rule: NaN is the greatest value, so MAX shows it and MIN shows it only where nothing else is
        assert np.all(np.isnan(got[2][where][at_nan - fol:at_nan + pre + 1])) and not np.any(np.isnan(got[1][where][ids == 0]))
    alone = hs_window_frames(dev, cols, [0, 0], 1, [(MIN, "between", value, 0, 0), (MAX, "between", value, 0, 0)], n)[1]
    assert np.isnan(alone[0].view(np.float32)[where][at_nan]) and np.array_equal(alone[0], alone[1])  # a frame of one row: the cell


def test_a_frame_of_zeros_of_both_signs(dev):
    value = upload(dev, np.array([-0.0, 0.0, -0.0, -0.0, 0.0], dtype=np.float32), T.FLOAT)
    for pre, fol in ((1, 1), (0, 1), (2, 0)):
        rc, got, flags = hs_window_frames(dev, [], [], 0, [(f, "between", value, pre, fol) for f in (SUM, MIN, MAX, AVG)], 5, n_keys=0)
        assert rc == 0 and flags == 0 and all(np.all(column.view(np.float32) == 0.0) for column in got)


@pytest.mark.parametrize("col_type", [T.INTEGER, T.FLOAT, T.TIMESTAMP])
def test_first_and_last_value_copy_the_cell_at_the_clamped_ends_bit_for_bit(dev, col_type):
    n = 2 * OB_TILE + 77
    rng = np.random.default_rng(31)
    ids = np.repeat(np.arange(n), rng.integers(1, 41, n))[:n]
    ids[OB_TILE - 30:OB_TILE + 30] = ids[OB_TILE - 30]  # one partition across the first tile boundary
    cols, part, order, _ = keyed(dev, rng, ids)
    column, bits = cells_of(dev, rng, n, col_type, special=col_type == T.FLOAT)  # FLOAT: NaNs with payloads, -0.0, a denormal
    if col_type == T.FLOAT:
        assert set(FLOATS.view(np.uint32).tolist()) >= set(bits.tolist())
    for pre, fol in ((0, 0), (1, 0), (0, 1), (3, 2), (45, 45), (K_MAX, 0), (0, K_MAX)):
        want = window_frame_exact(n, part, order, [0] * n, pre, fol)
        items = [(FIRST_VALUE, "between", column, pre, fol), (LAST_VALUE, "between", column, pre, fol)]
        rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and flags == 0, (said(dev), flags)
        differs(got[0], bits[np.asarray(want["first"])], f"{col_type}, ({pre}, {fol}), first_value")
        differs(got[1], bits[np.asarray(want["last"])], f"{col_type}, ({pre}, {fol}), last_value")


def test_a_frame_sum_beyond_i32_raises_only_where_a_frame_leaves_i32(dev):
    top = (1 << 31) - 1
    key = upload(dev, [0, 1, 2, 3], T.INTEGER)
    value = upload(dev, [top, 1, -5, 7], T.INTEGER)
    rc, got, flags = hs_window_frames(dev, [key], [0], 0, [(SUM, "between", value, 1, 0), (AVG, "between", value, 1, 0)], 4)
    assert rc == 0 and flags == INT_OVERFLOW, (said(dev), flags)
    assert got[0].view(np.int32).tolist() == [top, -(1 << 31), -4, 2]  # the second frame alone holds 2^31
    assert got[1].view(np.float32).tolist() == avg32([top, top + 1, -4, 2], [1, 2, 2, 2]).tolist()  # AVG divides the i64 sum
    value = upload(dev, [top, -5, 1, 7], T.INTEGER)  # the running sum of these never leaves i32, nor does any frame
    rc, got, flags = hs_window_frames(dev, [key], [0], 0, [(SUM, "between", value, 1, 1), (SUM, "between", value, 0, 0)], 4)
    assert rc == 0 and flags == 0 and got[0].view(np.int32).tolist() == [top - 5, top - 4, 3, 8] and got[1].view(np.int32).tolist() == [top, -5, 1, 7]


def test_two_f32_maxima_in_one_frame_raise_the_float_overflow(dev):
    big = np.finfo(np.float32).max
    value = upload(dev, [big, big, -big, 1.0], T.FLOAT)
    rc, got, flags = hs_window_frames(dev, [], [], 0, [(SUM, "between", value, 1, 0)], 4, n_keys=0)
    column = got[0].view(np.float32)
    assert rc == 0 and flags == FLT_OVERFLOW and column[0] == big and np.isinf(column[1]) and column[2] == 0.0 and column[3] == -big
    rc, got, flags = hs_window_frames(dev, [], [], 0, [(SUM, "between", value, 0, 0), (AVG, "between", value, 1, 0)], 4, n_keys=0)
    assert rc == 0 and flags == 0 and got[0].view(np.float32).tolist() == [big, big, -big, 1.0] and got[1].view(np.float32)[1] == big


def test_without_keys_the_frame_slides_over_the_input_order(dev):
    n = 2 * OB_TILE + 13
    cells = np.random.default_rng(4).integers(-50000, 50001, n)
    value = upload(dev, cells, T.INTEGER)
    items = [(SUM, "between", value, 2, 1), (COUNT, "between", None, 2, 1), (MAX, "between", value, 0, 3), (LAST_VALUE, "between", value, 0, 3)]
    rc, got, flags = hs_window_frames(dev, [], [], 0, items, n, n_keys=0)
    assert rc == 0 and flags == 0, said(dev)
    count, total, _, _ = numpy_frames(np.zeros(n, dtype=np.int64), cells, 2, 1)
    _, _, _, high = numpy_frames(np.zeros(n, dtype=np.int64), cells, 0, 3)
    differs(got[0].view(np.int32), total, "sum")
    differs(got[1].view(np.int32), count, "count")
    differs(got[2].view(np.int32), high, "max")
    differs(got[3].view(np.int32), cells[np.minimum(np.arange(n) + 3, n - 1)], "last_value")


def test_the_older_items_of_a_mixed_call_are_what_the_older_entries_return(dev):
    n = 3 * OB_TILE + 5
    rng = np.random.default_rng(41)
    cols, part, order, _ = keyed(dev, rng, np.repeat(np.arange(n), rng.integers(1, 41, n))[:n])
    cells = rng.integers(-999, 1000, n)
    value = upload(dev, cells, T.INTEGER)
    items = [(ROW_NUMBER, None, None), (SUM, "rows", value), (LAG, None, value, 0, 0, 2, 0xDEADBEEF), (SUM, "between", value, 3, 2),
             (NTILE, None, None, 0, 0, 3), (LAST_VALUE, "range", value), (LEAD, None, value, 0, 0, 1, 7), (AVG, "between", value, 0, 5)]
    rc, got, flags = hs_window_frames(dev, cols, [0, 0], 1, items, n)
    assert rc == 0 and flags == 0, (said(dev), flags)
    rc, ranks = hs_window(dev, cols, [0, 0], 1, [ROW_NUMBER], n)
    assert rc == 0 and np.array_equal(got[0].view(np.int32), ranks[0])
    rc, running, _ = hs_window_agg(dev, cols, [0, 0], 1, [(SUM, "rows", value)], n)
    assert rc == 0 and np.array_equal(got[1].view(np.int32), running[0])
    older = [(LAG, None, value, 2, 0xDEADBEEF), (NTILE, None, None, 3), (LAST_VALUE, "range", value), (LEAD, None, value, 1, 7)]
    rc, nav, _ = hs_window_nav(dev, cols, [0, 0], 1, older, n)
    assert rc == 0 and all(np.array_equal(got[k], theirs) for k, theirs in zip((2, 4, 5, 6), nav))
    want = window_frame_exact(n, part, order, py_values(cells, T.INTEGER), 3, 2)
    differs(got[3].view(np.int32), np.asarray(want["sum"]), "the sliding sum")
    want = window_frame_exact(n, part, order, py_values(cells, T.INTEGER), 0, 5)
    differs(got[7].view(np.float32), avg32(want["sum"], want["count"]), "the sliding average")


def test_refusals_are_codes_with_a_text_and_nothing_is_written(dev):
    col, stamps = upload(dev, [1, 2, 3], T.INTEGER), upload(dev, [1, 2, 3], T.TIMESTAMP)
    two = [col, col]

    def refused(items, code=1, keys=two, **how):
        rc, out, _ = hs_window_frames(dev, keys, [0] * len(keys), 1, items, 3, **how)
        assert rc == code and untouched(out), (rc, said(dev))
        return said(dev)

    assert b"12" in refused([(SUM, "between", col, 1, 1)], code=2, keys=[col] * 13)
    assert b"8" in refused([(SUM, "between", col, 1, 1)] * 9, code=2)
    assert b"function 13" in refused([(COUNT, "between", None, 1, 1), (13, "between", col, 1, 1)])
    assert b"item 1: frame 4" in refused([(COUNT, "between", None, 1, 1), (MIN, 4, col, 1, 1)])
    text = refused([(COUNT, "between", None, 1, 1), (AVG, "between", stamps, 1, 1)])
    assert b"item 1" in text and b"HS_I32 or HS_F32" in text
    for bad in (-1, 1 << 31):
        text = refused([(COUNT, "between", None, 0, 0), (SUM, "between", col, bad, 0)])
        assert b"item 1: preceding" in text and b"2^31" in text
        text = refused([(COUNT, "between", None, 0, 0), (LAST_VALUE, "between", col, 0, bad)])
        assert b"item 1: following" in text and b"2^31" in text
    assert b"item 1" in refused([(ROW_NUMBER, None, None), (SUM, "between", col, 1, 1)], no_preceding=True)
    assert b"following is null" in refused([(ROW_NUMBER, None, None), (MAX, "between", col, 1, 1)], no_following=True)
    for func in (ROW_NUMBER, LAG, LEAD, NTILE):
        text = refused([(COUNT, "between", None, 1, 1), (func, "between", col, 1, 1, 1, 0)])
        assert b"item 1: frame 3" in text and b"takes no frame" in text
    # the older entries go on refusing the frame
    rc, out, _ = hs_window_agg(dev, two, [0, 0], 1, [(COUNT, "rows", None), (MIN, 3, col)], 3)
    assert rc == 1 and b"hs_window_agg: item 1: frame 3" in said(dev) and out[0].tolist() == [-7] * 3
    rc, out, _ = hs_window_nav(dev, two, [0, 0], 1, [(COUNT, "rows", None), (LAST_VALUE, 3, col)], 3)
    assert rc == 1 and b"hs_window_nav: item 1: frame 3" in said(dev) and untouched(out)
    # ... and, as before, do not look at the frame of a function that takes none
    rc, out, _ = hs_window_nav(dev, two, [0, 0], 0, [(LAG, 3, col, 1, 0), (ROW_NUMBER, 3, None)], 3)
    assert rc == 0 and out[0].tolist() == [0, 1, 2] and out[1].tolist() == [1, 2, 3], said(dev)
    # accepted: no rows; only the offsets an item reads are looked at
    rc, out, _ = hs_window_frames(dev, two, [0, 0], 1, [(SUM, "between", col, 1, 1)], 0)
    assert rc == 0 and out[0].size == 0
    rc, out, _ = hs_window_frames(dev, two, [0, 0], 0, [(FIRST_VALUE, "between", col, 1, -9), (SUM, "rows", col, -3, -3)], 3,
                                  no_following=True)
    assert rc == 0 and out[0].tolist() == [1, 1, 2] and out[1].tolist() == [1, 3, 6]


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


@pytest.fixture(scope="module")
def api(engine):
    from minispark_amd.workloads import engine_api

    return engine_api(engine)


LINEITEM = lambda: load_golden("q1_multiblock")["paths"]["lineitem"]  # noqa: E731 - 6000 rows, 7 ship modes, several blocks


def with_frames(plain, items):
    """The model over the rows `plain` (the engine's own rows for the query without its window items): every item (name,
    function, argument name or None, partition names, [(order name, ascending)], n, m) becomes one more column.  The
    arguments used here are INTEGER, or FLOAT holding small whole numbers: every sum is exact, so its f32 is unique."""
    out = [dict(r) for r in plain]
    for name, kind, arg, partition, order, pre, fol in items:
        cells = [r[arg] for r in plain] if arg else [1] * len(plain)
        is_float = any(isinstance(c, float) for c in cells)
        model = window_frame_model(len(plain), [[r[p] for r in plain] for p in partition],
                                   [([r[o] for r in plain], ascending) for o, ascending in order], cells, pre, fol)
        for i, r in enumerate(out):
            if kind == "avg":
                r[name] = float(np.float32(np.float64(model["sum"][i]) / np.float64(model["count"][i])))
            elif kind in ("first_value", "last_value"):
                r[name] = cells[model[kind.split("_")[0]][i]]
            elif kind == "count" or not is_float:
                r[name] = int(model[kind][i])
            else:
                r[name] = float(np.float32(model[kind][i]))
    return out


def test_a_three_row_moving_average_per_key_with_qualify_by_sql_and_by_the_api(engine, api, monkeypatch):
    C_, F = api.Col, api.F
    plain = engine.sql(f"SELECT l_shipmode, l_orderkey, l_quantity FROM '{LINEITEM()}';").collect()
    assert isinstance(plain[0]["l_quantity"], float) and isinstance(plain[0]["l_orderkey"], int)
    spec = (["l_shipmode"], [("l_orderkey", True)])  # several lines per order: ties, in input order
    ranked = with_frames(plain, [("ma", "avg", "l_quantity", *spec, 2, 0), ("around", "sum", "l_orderkey", *spec, 1, 1),
                                 ("before", "first_value", "l_quantity", *spec, 2, 0)])
    want = [r for r in ranked if r["l_quantity"] > r["ma"]]
    calls = []
    window = type(engine.dev).window
    monkeypatch.setattr(type(engine.dev), "window", lambda self, *a: calls.append(
        [(i.func, i.frame, i.value, i.param, i.offsets) for i in a[3]]) or window(self, *a))
    over = "PARTITION BY l_shipmode ORDER BY l_orderkey"
    got = engine.sql(f"SELECT l_shipmode, l_orderkey, l_quantity, AVG(l_quantity) OVER ({over} ROWS BETWEEN 2 PRECEDING AND CURRENT ROW) "
                     f"AS ma, SUM(l_orderkey) OVER ({over} ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS around, "
                     f"FIRST_VALUE(l_quantity) OVER ({over} ROWS BETWEEN 2 PRECEDING AND CURRENT ROW) AS before "
                     f"FROM '{LINEITEM()}' QUALIFY l_quantity > ma;").collect()
    assert got == want and 1500 < len(got) < 4500
    assert calls == [[("avg", "between", 2, None, (2, 0)), ("sum", "between", 1, None, (1, 1)),
                      ("first_value", "between", 2, None, (2, 0))]]  # one sort, one call
    keys = dict(partition_by=[C_("l_shipmode")], order_by=[C_("l_orderkey")])
    frame = (api.DataFrame().table(LINEITEM()).select(C_("l_shipmode"), C_("l_orderkey"), C_("l_quantity"))
             .window(F.avg(C_("l_quantity")).over(**keys, rows=(2, 0)).alias("ma"),
                     F.sum(C_("l_orderkey")).over(**keys, rows=(1, 1)).alias("around"),
                     F.first_value(C_("l_quantity")).over(**keys, rows=(2, 0)).alias("before"))
             .qualify(C_("l_quantity") > C_("ma")))
    assert frame.collect() == got


def test_a_sliding_sum_over_group_by_results(engine, api):
    plain = engine.sql(f"SELECT l_shipmode, COUNT() AS n FROM '{LINEITEM()}' GROUP BY l_shipmode;").collect()
    want = with_frames(plain, [("pair", "sum", "n", [], [("l_shipmode", True)], 1, 0), ("top", "max", "n", [], [("l_shipmode", True)], 1, 1)])
    got = engine.sql("SELECT l_shipmode, COUNT() AS n, SUM(n) OVER (ORDER BY l_shipmode ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) AS pair, "
                     "MAX(n) OVER (ORDER BY l_shipmode ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS top "
                     f"FROM '{LINEITEM()}' GROUP BY l_shipmode;").collect()
    assert sorted(tuples(got)) == sorted(tuples(want)) and len(got) == 7
    assert sum(r["pair"] for r in got) == 2 * 6000 - max(got, key=lambda r: r["l_shipmode"])["n"]


def test_order_by_and_limit_on_top_of_a_sliding_item(engine, api):
    plain = engine.sql(f"SELECT l_returnflag, l_orderkey, l_extendedprice FROM '{LINEITEM()}';").collect()
    spec = (["l_returnflag"], [("l_orderkey", False), ("l_extendedprice", True)])
    ranked = with_frames(plain, [("low", "min", "l_orderkey", *spec, 0, 4), ("rows", "count", None, *spec, 3, 3),
                                 ("next", "last_value", "l_extendedprice", *spec, 0, 1)])
    want = sorted(tuples(ranked), key=lambda r: (r[4], -r[3], r[0], r[1], r[2]))[:11]
    over = "PARTITION BY l_returnflag ORDER BY l_orderkey DESC, l_extendedprice"
    got = engine.sql(f"SELECT l_returnflag, l_orderkey, l_extendedprice, MIN(l_orderkey) OVER ({over} ROWS BETWEEN CURRENT ROW AND 4 FOLLOWING) "
                     f"AS low, COUNT() OVER ({over} ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING) AS rows, LAST_VALUE(l_extendedprice) OVER ({over} "
                     f"ROWS BETWEEN CURRENT ROW AND 1 FOLLOWING) AS next FROM '{LINEITEM()}' "
                     "ORDER BY rows, low DESC, l_returnflag, l_orderkey, l_extendedprice LIMIT 11;").collect()
    assert tuples(got) == want and {r["rows"] for r in got} <= {4, 5}


def two_rank_frame(api, paths):
    # (l_orderkey, l_extendedprice, l_quantity) orders the rows of a ship mode totally: the frames do not depend on which
    # rank's rows the gathered result lists first
    C_, F = api.Col, api.F
    keys = dict(partition_by=[C_("l_shipmode")], order_by=[C_("l_orderkey").desc(), C_("l_extendedprice"), C_("l_quantity")])
    return (api.DataFrame().table(paths["lineitem"])
            .select(C_("l_shipmode"), C_("l_orderkey"), C_("l_extendedprice"), C_("l_quantity"))
            .window(F.row_number().over(**keys).alias("rn"), F.sum(C_("l_quantity")).over(**keys, rows=(1, 1)).alias("around"),
                    F.max(C_("l_orderkey")).over(**keys, rows=(0, 2)).alias("top"),
                    F.last_value(C_("l_orderkey")).over(**keys, rows=(0, 2)).alias("third"))
            .qualify(C_("rn") <= 5).order_by(C_("l_shipmode"), C_("rn")))


def test_two_ranks_slide_over_the_gathered_result_on_rank_0(tmp_path, engine, api):
    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_window_frames", "two_rank_frame", "q1_multiblock", out])
    one_rank = two_rank_frame(api, load_golden("q1_multiblock")["paths"]).collect()
    got = [tuple(r) for r in json.loads(out.read_text())]
    assert got == tuples(one_rank) and len(got) == 35
    # the order key descends: the frame's maximum is the row's own key, its last row's key is no greater
    assert all(math.isfinite(r[5]) and r[6] == r[1] and r[7] <= r[1] for r in got)
