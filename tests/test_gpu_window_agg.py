"""Window aggregates on the GPU.  At the C ABI (hs_window_agg) INTEGER results and FLOAT results over
values whose every f64 partial sum is exact must be EXACTLY those of the model (tests/window_agg_model.py); a FLOAT sum of
general values is held to the bound of an f64 sum under any association plus the final rounding, row by row.  End to end:
queries over the committed golden tables through engine.sql and the DataFrame API; the expected columns are the model
applied to the rows the same engine returns for the query without its window items."""

from __future__ import annotations

import json
import math

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, load_golden
from tests.ranks import run_ranks
from tests.test_gpu_distinct import py_values, tuples, upload
from tests.test_gpu_window import DENSE_RANK, OB_TILE, RANK, ROW_NUMBER, SIZES, hs_window, layouts
from tests.window_abi import call_window
from tests.window_agg_model import FRAMES, window_agg_model

pytestmark = pytest.mark.gpu

COUNT, SUM, AVG, MIN, MAX = 3, 4, 5, 6, 7
INT_OVERFLOW, FLT_OVERFLOW = 0x2, 0x4


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def hs_window_agg(dev, cols, descending, n_part, items, n, n_keys=None):
    """The entry point itself.  items = [(function, frame name or None, value column or None)] -> (return code, [one
    array per item, input order: float32 where the item's value is FLOAT, else int32], the status word)."""
    from minispark_amd import hipspark as hs

    rc, got, flags = call_window(dev, "hs_window_agg", cols, descending, n_part, items, n, n_keys)
    is_float = lambda f, v: f == AVG or (f in (SUM, MIN, MAX) and v is not None and v.kind == hs.F32)  # noqa: E731
    return rc, [o.view(np.float32 if is_float(f, v) else np.int32) for (f, _, v), o in zip(items, got)], flags


def keys_of(dev, ids, values):
    """PARTITION BY an INTEGER, ORDER BY an INTEGER ascending (test_gpu_window's shape_i32_i32): uploaded columns and the
    model's view of them."""
    partition, order = [(ids * 7 - 3, T.INTEGER)], [(values - 50, T.INTEGER, True)]
    cols = [upload(dev, v, t) for v, t in partition] + [upload(dev, v, t) for v, t, _ in order]
    return cols, [py_values(v, t) for v, t in partition], [(py_values(v, t), a) for v, t, a in order]


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def avg32(sums, counts):
    return (np.asarray(sums, dtype=np.float64) / np.asarray(counts, dtype=np.float64)).astype(np.float32)


def exact_checks(dev, n, cols, desc, n_part, model_part, model_order, cells, col_type, where):
    """COUNT / SUM / MIN / MAX / AVG of one argument column under all three frames against the model, exactly (zeros and
    every other value by VALUE: the results hold no NaN)."""
    value = upload(dev, cells, col_type)
    cells = py_values(cells, col_type)
    calls = [[(f, frame, value) for f in (COUNT, SUM, MIN, MAX, AVG)] for frame in FRAMES]
    for frame, items in zip(FRAMES, calls):
        rc, got, flags = hs_window_agg(dev, cols, desc, n_part, items, n)
        assert rc == 0 and flags == 0, (dev._raw_lib.hs_last_error(), flags)
        want = window_agg_model(n, model_part, model_order, cells, frame)
        cast = f32 if col_type == T.FLOAT else (lambda x: np.asarray(x, dtype=np.int64))
        expected = {COUNT: np.asarray(want["count"], dtype=np.int64), SUM: cast(want["sum"]), MIN: cast(want["min"]),
                    MAX: cast(want["max"]), AVG: avg32(want["sum"], want["count"])}
        for (f, _, _), column in zip(items, got):
            bad = np.nonzero(column != expected[f])[0]
            assert bad.size == 0, (f"{where}, {frame}: function {f} differs at {bad.size} of {n} rows, first row {bad[0]}: got "
                                   f"{column[bad[0]]!r}, want {expected[f][bad[0]]!r}")


@pytest.mark.parametrize("n", SIZES)
def test_integer_aggregates_are_exactly_the_model(dev, n):
    if n == 0:
        col = upload(dev, [0], T.INTEGER)
        rc, got, flags = hs_window_agg(dev, [col, col], [0, 0], 1, [(SUM, "range", col), (COUNT, "rows", None)], 0)
        assert rc == 0 and flags == 0 and got[0].size == 0
        return
    rng = np.random.default_rng(n)
    for name, ids, values in layouts(n):
        cols, part, order = keys_of(dev, ids, values)
        exact_checks(dev, n, cols, [0, 0], 1, part, order, rng.integers(-50000, 50001, n), T.INTEGER, name)  # |sum| < 2^31


@pytest.mark.parametrize("n", [s for s in SIZES if s])
def test_float_aggregates_of_exactly_summable_values_are_bit_exact(dev, n):
    """k / 64 with |k| < 2^20: every f64 partial sum of these rows is exact, so the f32 result does not depend on the
    association."""
    rng = np.random.default_rng(7 * n)
    for name, ids, values in layouts(n):
        cols, part, order = keys_of(dev, ids, values)
        cells = (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32)
        exact_checks(dev, n, cols, [0, 0], 1, part, order, cells, T.FLOAT, name)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("n", sorted(SIZES)[-3:])
def test_float_sums_of_general_values_stay_inside_the_f64_bound(dev, n):
    """|got - X| <= (m - 1) 2^-52 sum|x| + ulp_f32(max(|got|, |X|)) / 2 for EVERY row: X the exact frame sum, m its rows.
    The first term bounds an f64 sum under any association (gamma_k <= 2ku), the second is the rounding to f32.  AVG: the
    same divided by m, plus its own half ulp.  And the same call twice gives the same bits."""
    rng = np.random.default_rng(3 * n)
    for name, ids, values in layouts(n):
        cols, part, order = keys_of(dev, ids, values)
        cells = (rng.uniform(-1e6, 1e6, n) * 2.0 ** rng.integers(-30, 1, n)).astype(np.float32)
        value = upload(dev, cells, T.FLOAT)
        items = [(f, frame, value) for frame in FRAMES for f in (SUM, AVG)]
        rc, got, flags = hs_window_agg(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
        rc, again, _ = hs_window_agg(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))
        for k, frame in enumerate(FRAMES):
            want = window_agg_model(n, part, order, py_values(cells, T.FLOAT), frame)
            X, m, mass = np.asarray(want["sum"]), np.asarray(want["count"], dtype=np.float64), np.asarray(want["abs"])
            s, a = got[2 * k].astype(np.float64), got[2 * k + 1].astype(np.float64)
            bound = (m - 1) * 2.0 ** -52 * mass + 0.5 * ulp32(np.maximum(np.abs(s), np.abs(X)))
            off = np.abs(s - X)
            print(f"n={n} {name} {frame}: SUM worst |got - X| / bound = {np.max(off / bound):.3g}")
            assert np.all(off <= bound), (name, frame, int(np.argmax(off - bound)))
            bound_avg = bound / m + 0.5 * ulp32(np.maximum(np.abs(a), np.abs(X / m)))
            off = np.abs(a - X / m)
            print(f"n={n} {name} {frame}: AVG worst |got - X/m| / bound = {np.max(off / bound_avg):.3g}")
            assert np.all(off <= bound_avg), (name, frame, int(np.argmax(off - bound_avg)))


def test_ranking_items_of_a_mixed_call_are_what_hs_window_returns(dev):
    n = SIZES[-1]
    _name, ids, values = layouts(n)[-1]
    cols, part, order = keys_of(dev, ids, values)
    cells = np.random.default_rng(1).integers(-999, 1000, n)
    value = upload(dev, cells, T.INTEGER)
    items = [(ROW_NUMBER, None, None), (SUM, "range", value), (RANK, None, None), (COUNT, "range", None), (DENSE_RANK, None, None)]
    rc, got, flags = hs_window_agg(dev, cols, [0, 0], 1, items, n)
    assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
    rc, ranks = hs_window(dev, cols, [0, 0], 1, [ROW_NUMBER, RANK, DENSE_RANK], n)
    assert rc == 0
    for mine, theirs in zip((got[0], got[2], got[4]), ranks):
        assert np.array_equal(mine, theirs)
    want = window_agg_model(n, part, order, py_values(cells, T.INTEGER), "range")
    assert np.array_equal(got[1], np.asarray(want["sum"])) and np.array_equal(got[3], np.asarray(want["count"]))


def test_a_two_word_key_with_a_coded_partition_column_and_a_descending_order_key(dev):
    n = 3 * OB_TILE + 77
    rng = np.random.default_rng(21)
    _name, ids, values = layouts(n)[-1]
    names = [b"p%03d" % (i % 5) for i in ids]
    stamps = (ids.astype(np.int64) << 21) + (1 << 44)
    cols = [dev.dict_encode(upload(dev, names, T.STRING)), upload(dev, stamps, T.TIMESTAMP), upload(dev, values, T.INTEGER)]
    assert cols[0] is not None and cols[0].dict is not None
    cells = rng.integers(-50000, 50001, n)
    value = upload(dev, cells, T.INTEGER)
    part, order = [py_values(names, T.STRING), py_values(stamps, T.TIMESTAMP)], [(py_values(values, T.INTEGER), False)]
    for frame in FRAMES:
        rc, got, flags = hs_window_agg(dev, cols, [0, 0, 1], 2, [(SUM, frame, value), (MAX, frame, value), (COUNT, frame, None)], n)
        assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
        want = window_agg_model(n, part, order, py_values(cells, T.INTEGER), frame)
        for column, k in zip(got, ("sum", "max", "count")):
            assert np.array_equal(column, np.asarray(want[k])), (frame, k)


def test_aggregates_across_a_round_of_the_tile_scan(dev):
    """The tile-carry kernel takes OB_TILE summaries per round: rows beyond OB_TILE tiles lie in its second round, and the
    64-bit fold's carry crosses it.  Three partitions in order, the middle one starting in the first round and ending in
    the second; the order key is the position, so every row is its own peer group and RANGE is ROWS.  Cells in [-3, 3]:
    no sum leaves i32, and the FLOAT sums (|sum| < 2^24) are exact under any association.  Expected values are numpy's
    segmented cumsum / accumulate per partition, compared exactly."""
    n = OB_TILE * OB_TILE + 3 * OB_TILE + 5
    rng = np.random.default_rng(22)
    position = np.arange(n)
    ids = np.where(position < 1000, 0, np.where(position < n - 700, 1, 2))
    cells = rng.integers(-3, 4, n)
    cols = [upload(dev, ids, T.INTEGER), upload(dev, position, T.INTEGER)]
    value, value_f = upload(dev, cells, T.INTEGER), upload(dev, cells.astype(np.float32), T.FLOAT)
    running = {f: np.empty(n, dtype=np.int64) for f in (COUNT, SUM, MIN, MAX)}
    whole = {f: np.empty(n, dtype=np.int64) for f in (COUNT, SUM, MIN, MAX)}
    for lo, hi in ((0, 1000), (1000, n - 700), (n - 700, n)):
        part = cells[lo:hi]
        running[COUNT][lo:hi] = np.arange(1, hi - lo + 1)
        running[SUM][lo:hi] = np.cumsum(part)
        running[MIN][lo:hi] = np.minimum.accumulate(part)
        running[MAX][lo:hi] = np.maximum.accumulate(part)
        for f in running:
            whole[f][lo:hi] = running[f][hi - 1]
    for frame in FRAMES:
        want = whole if frame == "partition" else running
        items = [(COUNT, frame, None), (SUM, frame, value), (MIN, frame, value), (MAX, frame, value), (SUM, frame, value_f)]
        rc, got, flags = hs_window_agg(dev, cols, [0, 0], 1, items, n)
        assert rc == 0 and flags == 0, (dev._raw_lib.hs_last_error(), flags)
        expected = [want[COUNT], want[SUM], want[MIN], want[MAX], want[SUM].astype(np.float32)]
        for (f, _, v), column, exp in zip(items, got, expected):
            bad = np.nonzero(column != exp)[0]
            assert bad.size == 0, (f"{frame}: function {f} of kind {v.kind if v is not None else None} differs at {bad.size} of "
                                   f"{n} rows, first row {bad[0]}: got {column[bad[0]]!r}, want {exp[bad[0]]!r}")


def test_without_keys_the_rows_frame_is_a_running_sum_in_input_order(dev):
    n = 2 * OB_TILE + 13
    cells = np.random.default_rng(4).integers(-50000, 50001, n)
    value = upload(dev, cells, T.INTEGER)
    rc, got, flags = hs_window_agg(dev, [], [], 0, [(SUM, "rows", value), (COUNT, "rows", None), (SUM, "range", value)], n, n_keys=0)
    assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
    assert np.array_equal(got[0], np.cumsum(cells)) and np.array_equal(got[1], np.arange(1, n + 1))
    assert np.array_equal(got[2], np.full(n, cells.sum()))  # no order key: every row a peer of every other


def test_a_running_prefix_beyond_i32_raises_and_a_partition_total_inside_does_not(dev):
    cells = [(1 << 31) - 1, 1, -5]
    key, value = upload(dev, [0, 1, 2], T.INTEGER), upload(dev, cells, T.INTEGER)
    for frame in ("rows", "range"):
        rc, got, flags = hs_window_agg(dev, [key], [0], 0, [(SUM, frame, value)], 3)
        assert rc == 0 and flags == INT_OVERFLOW and got[0][0] == (1 << 31) - 1 and got[0][2] == (1 << 31) - 5
    rc, got, flags = hs_window_agg(dev, [key], [0], 0, [(SUM, "partition", value), (AVG, "rows", value)], 3)
    assert rc == 0 and flags == 0 and got[0].tolist() == [(1 << 31) - 5] * 3
    assert got[1].tolist() == avg32([cells[0], cells[0] + 1, cells[0] - 4], [1, 2, 3]).tolist()  # AVG divides the i64 sum


def test_two_f32_maxima_raise_the_float_overflow(dev):
    big = np.finfo(np.float32).max
    value = upload(dev, [big, big, -big], T.FLOAT)
    rc, got, flags = hs_window_agg(dev, [], [], 0, [(SUM, "rows", value)], 3, n_keys=0)
    assert rc == 0 and flags == FLT_OVERFLOW and got[0][0] == big and np.isinf(got[0][1]) and got[0][2] == big
    rc, got, flags = hs_window_agg(dev, [], [], 0, [(SUM, "partition", value), (AVG, "rows", value)], 3, n_keys=0)
    assert rc == 0 and flags == 0 and got[0].tolist() == [big] * 3 and got[1][1] == big


def test_nan_and_infinities_stay_inside_their_partition_across_a_tile_boundary(dev):
    n = OB_TILE + 100
    position = np.arange(n)
    ids = np.where(position < OB_TILE - 10, 0, np.where(position < OB_TILE + 10, 1, 2))
    rng = np.random.default_rng(8)
    cells = (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32)
    middle = np.nonzero(ids == 1)[0]
    cells[middle] = np.resize(np.array([np.nan, np.inf, 2.5, -np.inf], dtype=np.float32), middle.size)
    shuffle = rng.permutation(n)
    ids, cells = ids[shuffle], cells[shuffle]
    key, value = upload(dev, ids, T.INTEGER), upload(dev, cells, T.FLOAT)
    for frame in ("partition", "rows"):
        rc, got, flags = hs_window_agg(dev, [key], [0], 1, [(f, frame, value) for f in (SUM, MIN, MAX, AVG)], n)
        assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
        want = window_agg_model(n, [py_values(ids, T.INTEGER)], [], py_values(cells, T.FLOAT), frame)
        outside = ids != 1
        assert np.all(np.isfinite(got[0][outside])) and np.array_equal(got[0][outside], f32(want["sum"])[outside])
        assert np.array_equal(got[3][outside], avg32(want["sum"], want["count"])[outside])
        for column, k in zip(got[:3], ("sum", "min", "max")):  # inside: NaN where the model has one, else its value
            expected = f32(want[k])
            assert np.array_equal(np.isnan(column), np.isnan(expected)) and np.array_equal(column[~np.isnan(expected)],
                                                                                            expected[~np.isnan(expected)]), (frame, k)
    whole = hs_window_agg(dev, [key], [0], 1, [(MAX, "partition", value), (MIN, "partition", value), (SUM, "partition", value)], n)[1]
    assert np.all(np.isnan(whole[0][ids == 1])) and np.all(whole[1][ids == 1] == -np.inf) and np.all(np.isnan(whole[2][ids == 1]))


def test_a_frame_of_zeros_of_both_signs(dev):
    value = upload(dev, np.array([-0.0, 0.0, -0.0, -0.0], dtype=np.float32), T.FLOAT)
    rc, got, flags = hs_window_agg(dev, [], [], 0, [(f, "rows", value) for f in (SUM, MIN, MAX, AVG)], 4, n_keys=0)
    assert rc == 0 and flags == 0 and all(np.all(column == 0.0) for column in got)


def test_refusals_are_codes_with_a_text_and_nothing_is_written(dev):
    col, stamps = upload(dev, [1, 2, 3], T.INTEGER), upload(dev, [1, 2, 3], T.TIMESTAMP)
    lib = dev._raw_lib
    rc, out, _ = hs_window_agg(dev, [col] * 13, [0] * 13, 1, [(SUM, "rows", col)], 3)
    assert rc == 2 and b"12" in lib.hs_last_error() and out[0].tolist() == [-7] * 3
    rc, out, _ = hs_window_agg(dev, [col, col], [0, 0], 1, [(SUM, "rows", col)] * 9, 3)
    assert rc == 2 and b"8" in lib.hs_last_error()
    rc, out, _ = hs_window_agg(dev, [col, col], [0, 0], 1, [(COUNT, "rows", None), (8, "rows", col)], 3)
    assert rc == 1 and b"function 8" in lib.hs_last_error() and out[0].tolist() == [-7] * 3
    rc, out, _ = hs_window_agg(dev, [col, col], [0, 0], 1, [(COUNT, "rows", None), (MIN, 3, col)], 3)
    assert rc == 1 and b"item 1: frame 3" in lib.hs_last_error() and out[0].tolist() == [-7] * 3
    rc, out, _ = hs_window_agg(dev, [col, col], [0, 0], 1, [(COUNT, "rows", None), (AVG, "rows", stamps)], 3)
    assert rc == 1 and b"item 1" in lib.hs_last_error() and b"HS_I32 or HS_F32" in lib.hs_last_error()
    assert out[0].tolist() == [-7] * 3
    rc, out, _ = hs_window_agg(dev, [col], [0], 1, [(SUM, "rows", col), (RANK, None, None)], 3)
    assert rc == 1 and b"order key" in lib.hs_last_error()
    rc, out, _ = hs_window_agg(dev, [col] * 12, [0] * 12, 11, [(SUM, "range", col), (COUNT, "partition", None)], 3)
    assert rc == 0 and out[0].tolist() == [1, 2, 3] and out[1].tolist() == [1, 1, 1]


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


def with_aggregates(plain, items):
    """The model over the rows `plain` (the engine's own rows for the query without its window items): every item (name,
    function, argument name or None, partition names, [(order name, ascending)], frame) becomes one more column.  The
    arguments used here are INTEGER, or FLOAT holding small whole numbers: every sum is exact, so its f32 is unique."""
    out = [dict(r) for r in plain]
    for name, kind, arg, partition, order, frame in items:
        cells = [r[arg] for r in plain] if arg else [1] * len(plain)
        is_float = any(isinstance(c, float) for c in cells)
        model = window_agg_model(len(plain), [[r[p] for r in plain] for p in partition],
                                 [([r[o] for r in plain], ascending) for o, ascending in order], cells, frame)
        for i, r in enumerate(out):
            if kind == "avg":
                r[name] = float(np.float32(np.float64(model["sum"][i]) / np.float64(model["count"][i])))
            elif kind == "count" or not is_float:
                r[name] = int(model[kind][i])
            else:
                r[name] = float(np.float32(model[kind][i]))
    return out


def test_a_share_of_a_partition_total(engine, api):
    C_, F = api.Col, api.F
    plain = engine.sql(f"SELECT l_shipmode, l_orderkey, l_quantity FROM '{LINEITEM()}';").collect()
    assert isinstance(plain[0]["l_quantity"], float) and isinstance(plain[0]["l_orderkey"], int)
    want = with_aggregates(plain, [("total", "sum", "l_quantity", ["l_shipmode"], [], "partition"),
                                   ("n", "count", None, ["l_shipmode"], [], "partition"),
                                   ("keys", "sum", "l_orderkey", ["l_shipmode"], [], "partition")])
    got = engine.sql("SELECT l_shipmode, l_orderkey, l_quantity, SUM(l_quantity) OVER (PARTITION BY l_shipmode) AS total, "
                     "COUNT() OVER (PARTITION BY l_shipmode) AS n, SUM(l_orderkey) OVER (PARTITION BY l_shipmode) AS keys "
                     f"FROM '{LINEITEM()}';").collect()
    assert len(got) == 6000 and got == want and len({r["total"] for r in got}) == 7
    assert isinstance(got[0]["total"], float) and isinstance(got[0]["keys"], int)
    frame = (api.DataFrame().table(LINEITEM()).select(C_("l_shipmode"), C_("l_orderkey"), C_("l_quantity"))
             .window(F.sum(C_("l_quantity")).over(partition_by=[C_("l_shipmode")]).alias("total"),
                     F.count().over(partition_by=[C_("l_shipmode")]).alias("n"),
                     F.sum(C_("l_orderkey")).over(partition_by=[C_("l_shipmode")]).alias("keys")))
    assert frame.collect() == got


def test_a_running_sum_with_ties_under_range_and_rows(engine, api):
    plain = engine.sql(f"SELECT l_returnflag, l_quantity, l_orderkey FROM '{LINEITEM()}';").collect()
    spec = (["l_returnflag"], [("l_quantity", False)])
    want = with_aggregates(plain, [("peers", "sum", "l_quantity", *spec, "range"), ("upto", "sum", "l_quantity", *spec, "rows"),
                                   ("low", "min", "l_orderkey", *spec, "rows"), ("mean", "avg", "l_orderkey", *spec, "range")])
    over = "PARTITION BY l_returnflag ORDER BY l_quantity DESC"
    got = engine.sql(f"SELECT l_returnflag, l_quantity, l_orderkey, SUM(l_quantity) OVER ({over}) AS peers, "
                     f"SUM(l_quantity) OVER ({over} ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW) AS upto, "
                     f"MIN(l_orderkey) OVER ({over} ROWS UNBOUNDED PRECEDING) AS low, "
                     f"AVG(l_orderkey) OVER ({over} RANGE UNBOUNDED PRECEDING) AS mean FROM '{LINEITEM()}';").collect()
    assert got == want and any(r["peers"] != r["upto"] for r in got)  # 50 quantities over 6000 rows: ties everywhere


def test_rows_above_their_partitions_average(engine, api):
    plain = engine.sql(f"SELECT l_shipmode, l_quantity FROM '{LINEITEM()}';").collect()
    ranked = with_aggregates(plain, [("avg_l_quantity", "avg", "l_quantity", ["l_shipmode"], [], "partition")])
    want = [r for r in ranked if r["l_quantity"] > r["avg_l_quantity"]]
    got = engine.sql("SELECT l_shipmode, l_quantity, AVG(l_quantity) OVER (PARTITION BY l_shipmode) "
                     f"FROM '{LINEITEM()}' QUALIFY l_quantity > avg_l_quantity;").collect()
    assert got == want and 2000 < len(got) < 4000


def test_a_running_sum_over_group_by_results(engine, api):
    plain = engine.sql(f"SELECT l_shipmode, COUNT() AS n FROM '{LINEITEM()}' GROUP BY l_shipmode;").collect()
    want = with_aggregates(plain, [("running", "sum", "n", [], [("l_shipmode", True)], "range")])
    got = engine.sql("SELECT l_shipmode, COUNT() AS n, SUM(n) OVER (ORDER BY l_shipmode) AS running "
                     f"FROM '{LINEITEM()}' GROUP BY l_shipmode;").collect()
    assert sorted(tuples(got)) == sorted(tuples(want)) and len(got) == 7 and max(r["running"] for r in got) == 6000


def test_an_aggregate_next_to_row_number_with_distinct_order_by_and_limit(engine, api, monkeypatch):
    from tests.test_gpu_window import with_windows

    plain = engine.sql(f"SELECT l_shipmode, l_returnflag FROM '{LINEITEM()}';").collect()
    ranked = with_windows(plain, [("rn", "row_number", ["l_shipmode"], [("l_returnflag", True)])])
    ranked = with_aggregates(ranked, [("c", "count", None, ["l_shipmode"], [("l_returnflag", True)], "range")])
    kept = list(dict.fromkeys(tuples(r for r in ranked if r["rn"] <= 400)))
    want = sorted(kept, key=lambda r: (-r[3], r[0], r[2]))[:9]
    calls = []
    window = type(engine.dev).window
    monkeypatch.setattr(type(engine.dev), "window", lambda self, *a: calls.append([i.func for i in a[3]]) or window(self, *a))
    over = "OVER (PARTITION BY l_shipmode ORDER BY l_returnflag)"
    got = engine.sql(f"SELECT DISTINCT l_shipmode, l_returnflag, ROW_NUMBER() {over} AS rn, COUNT() {over} AS c "
                     f"FROM '{LINEITEM()}' QUALIFY rn <= 400 ORDER BY c DESC, l_shipmode, rn LIMIT 9;").collect()
    assert tuples(got) == want and calls == [["row_number", "count"]]  # one spec: one sort, one call


def two_rank_frame(api, paths):
    # (l_orderkey, l_extendedprice, l_quantity) orders the rows of a ship mode totally: the running sums do not depend on
    # which rank's rows the gathered result lists first
    C_, F = api.Col, api.F
    keys = dict(partition_by=[C_("l_shipmode")], order_by=[C_("l_orderkey").desc(), C_("l_extendedprice"), C_("l_quantity")])
    return (api.DataFrame().table(paths["lineitem"])
            .select(C_("l_shipmode"), C_("l_orderkey"), C_("l_extendedprice"), C_("l_quantity"))
            .window(F.row_number().over(**keys).alias("rn"), F.sum(C_("l_quantity")).over(**keys, rows=True).alias("upto"),
                    F.max(C_("l_orderkey")).over(partition_by=[C_("l_shipmode")]).alias("top"))
            .qualify(C_("rn") <= 5).order_by(C_("l_shipmode"), C_("rn")))


def test_two_ranks_aggregate_the_gathered_result_on_rank_0(tmp_path, engine, api):
    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_window_agg", "two_rank_frame", "q1_multiblock", out])
    one_rank = two_rank_frame(api, load_golden("q1_multiblock")["paths"]).collect()
    got = [tuple(r) for r in json.loads(out.read_text())]
    assert got == tuples(one_rank) and len(got) == 35
    assert all(math.isfinite(r[5]) and r[6] >= r[1] for r in got)
