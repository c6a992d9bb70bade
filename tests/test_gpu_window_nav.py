"""Window navigation on the GPU.  LAG / LEAD / FIRST_VALUE / LAST_VALUE copy cells, so at the C ABI
(hs_window_nav) every output cell is compared BIT FOR BIT (uint32 / uint64 views) with the cell the model
(tests/window_nav_model.py) points at, and NTILE with the model's bucket.  End to end: queries over the committed golden
tables through engine.sql and the DataFrame API; the expected columns are the model applied to the rows the same engine
returns for the query without its window items."""

from __future__ import annotations

import json
from datetime import datetime

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, load_golden
from tests.ranks import run_ranks
from tests.test_gpu_distinct import py_values, tuples, upload
from tests.test_gpu_window import (DENSE_RANK, FLOATS, OB_TILE, ROW_NUMBER, SIZES, hs_window, layouts, shape_i32_i32,
                                   shape_no_partition, shape_timestamp_i32)
from tests.test_gpu_window_agg import AVG, COUNT, SUM, hs_window_agg
from tests.window_abi import SENTINEL, call_window
from tests.window_nav_model import FRAMES, window_nav_model, window_nav_plan

pytestmark = pytest.mark.gpu

LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTILE = 8, 9, 10, 11, 12
NAMES = {LAG: "lag", LEAD: "lead", FIRST_VALUE: "first_value", LAST_VALUE: "last_value", NTILE: "ntile"}
K_MAX = (1 << 31) - 1
# a default per cell type that no cell of the tests holds: an INTEGER, a NaN with a payload, a TIMESTAMP
DEFAULTS = {T.INTEGER: 0xDEADBEEF, T.FLOAT: 0x7FC12345, T.TIMESTAMP: 0x8000000000000123}


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def hs_window_nav(dev, cols, descending, n_part, items, n, n_keys=None, no_params=False, no_defaults=False):
    """The entry point itself.  items = [(function, frame name / code or None, value column or None, k or n, default bits)]
    -> (return code, [one array per item, input order: the cells' bits as uint32, uint64 for an 8-byte argument], the
    status word).  Every output is allocated with a sentinel and SLACK cells behind the rows, which must stay untouched."""
    omit = [name for name, off in (("params", no_params), ("defaults", no_defaults)) if off]
    return call_window(dev, "hs_window_nav", cols, descending, n_part, items, n, n_keys, omit)


def untouched(out):
    return all(np.all(o.view(np.int64 if o.dtype == np.uint64 else np.int32) == SENTINEL) for o in out)


def cells_of(dev, rng, n, col_type, special=False):
    """An argument column of `col_type` -> (the uploaded column, its cells' bits).  FLOAT cells are arbitrary bit patterns
    - NaNs with payloads, denormals, infinities among them -, or with `special` the nine of test_gpu_window's FLOATS."""
    if col_type == T.TIMESTAMP:
        bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        return upload(dev, bits.view(np.int64), T.TIMESTAMP), bits
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if special:
        bits = FLOATS.view(np.uint32)[rng.integers(0, len(FLOATS), n)]
    if col_type == T.FLOAT:
        return upload(dev, bits.view(np.float32), T.FLOAT), bits
    return upload(dev, bits.view(np.int32), T.INTEGER), bits


def offsets(n):
    ks = [0, 1, 7, 8, 9, 63, 64, 65, OB_TILE - 1, OB_TILE, OB_TILE + 1, n - 1, n, K_MAX]
    return list(dict.fromkeys(k for k in ks if k >= 0))


BUCKETS = [1, 2, 3, 7, 64, K_MAX]


def all_items(n):
    """(function, frame, k or n) of every item the boundary tests ask for"""
    return ([(f, None, k) for k in offsets(n) for f in (LAG, LEAD)] + [(f, frame, None) for frame in FRAMES for f in (FIRST_VALUE, LAST_VALUE)]
            + [(NTILE, None, b) for b in BUCKETS])


def check_nav(dev, n, cols, desc, n_part, model_part, model_order, typed, specs, where, n_keys=None):
    """`specs` over every argument column of `typed` = [(column type, uploaded column, bits)], eight items a call, against
    the model bit for bit.  The model runs once per item over the ROW NUMBERS: a copy is the same whatever the cells are."""
    sources, plan = [], window_nav_plan(n, model_part, model_order)
    for f, frame, p in specs:
        if f == NTILE:
            sources.append(window_nav_model(n, model_part, model_order, None, "ntile", buckets=p, plan=plan))
        else:
            sources.append(window_nav_model(n, model_part, model_order, np.arange(n, dtype=np.int64), NAMES[f], frame=frame, k=p,
                                            default=-1, plan=plan))
    for col_type, column, bits in typed:
        for at in range(0, len(specs), 8):
            batch = specs[at:at + 8]
            items = [(f, frame, None if f == NTILE else column, p, DEFAULTS[col_type]) for f, frame, p in batch]
            rc, got, flags = hs_window_nav(dev, cols, desc, n_part, items, n, n_keys=n_keys)
            assert rc == 0 and flags == 0, (dev._raw_lib.hs_last_error(), flags)
            for (f, frame, p), src, column_got in zip(batch, sources[at:at + 8], got):
                if f == NTILE:
                    want = src.astype(np.uint32)
                else:
                    want = np.where(src >= 0, bits[np.maximum(src, 0)], bits.dtype.type(DEFAULTS[col_type]))
                assert column_got.dtype == want.dtype
                bad = np.nonzero(column_got != want)[0]
                assert bad.size == 0, (f"{where}, {col_type}: {NAMES[f]} frame={frame} k/n={p} differs at {bad.size} of {n} rows, "
                                       f"first row {bad[0]}: got {column_got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def keys_for(dev, shape, ids, values, coded=()):
    """One of test_gpu_window's key shapes -> (uploaded key columns, descending flags, n_part, the model's partition and
    order)"""
    partition, order = shape["partition"], shape["order"]
    cols = [upload(dev, v, t) for v, t in partition] + [upload(dev, v, t) for v, t, _ in order]
    for k in coded:
        cols[k] = dev.dict_encode(cols[k])
        assert cols[k] is not None and cols[k].dict is not None
    desc = [0] * len(partition) + [0 if a else 1 for _, _, a in order]
    return cols, desc, len(partition), [py_values(v, t) for v, t in partition], [(py_values(v, t), a) for v, t, a in order]


@pytest.mark.parametrize("n", SIZES)
def test_every_function_at_every_tile_boundary_is_the_model_bit_for_bit(dev, n):
    if n == 0:
        col, stamps = upload(dev, [0], T.INTEGER), upload(dev, [0], T.TIMESTAMP)
        items = [(LAG, None, col, 1, 5), (LEAD, None, stamps, 0, 5), (LAST_VALUE, "range", col), (NTILE, None, None, 4)]
        rc, got, flags = hs_window_nav(dev, [col, col], [0, 0], 1, items, 0)
        assert rc == 0 and flags == 0 and all(g.size == 0 for g in got)
        return
    rng = np.random.default_rng(n)
    typed = [(ty, *cells_of(dev, rng, n, ty)) for ty in (T.INTEGER, T.FLOAT, T.TIMESTAMP)]
    for name, ids, values in layouts(n):
        cols, desc, n_part, part, order = keys_for(dev, shape_i32_i32(ids, values), ids, values)
        check_nav(dev, n, cols, desc, n_part, part, order, typed, all_items(n), name)


def test_a_two_word_key_a_coded_partition_with_a_descending_order_key_and_no_partition(dev):
    n = 3 * OB_TILE + 77
    rng = np.random.default_rng(21)
    _name, ids, values = layouts(n)[-1]
    typed = [(ty, *cells_of(dev, rng, n, ty)) for ty in (T.INTEGER, T.TIMESTAMP)]
    specs = [(LAG, None, 1), (LEAD, None, 1), (LEAD, None, 9), (LAG, None, 64), (FIRST_VALUE, "range", None), (LAST_VALUE, "range", None),
             (LAST_VALUE, "partition", None), (NTILE, None, 3)]
    check_nav(dev, n, *keys_for(dev, shape_timestamp_i32(ids, values), ids, values), typed, specs, "timestamp_i32")
    coded = dict(partition=[([b"p%03d" % (i % 5) for i in ids], T.STRING), ((ids.astype(np.int64) << 21) + (1 << 44), T.TIMESTAMP)],
                 order=[(values, T.INTEGER, False)])
    check_nav(dev, n, *keys_for(dev, coded, ids, values, coded=(0,)), typed, specs, "coded partition, descending order")
    check_nav(dev, n, *keys_for(dev, shape_no_partition(ids, values), ids, values), typed, specs, "no partition")


def test_without_keys_lag_and_lead_shift_the_input_and_ntile_buckets_it(dev):
    n = 2 * OB_TILE + 13
    rng = np.random.default_rng(4)
    for ty in (T.INTEGER, T.TIMESTAMP):
        column, bits = cells_of(dev, rng, n, ty)
        d = bits.dtype.type(DEFAULTS[ty])
        items = [(LAG, None, column, 3, d), (LEAD, None, column, OB_TILE + 1, d), (LEAD, None, column, n, d), (FIRST_VALUE, "rows", column),
                 (LAST_VALUE, "range", column), (LAST_VALUE, "rows", column), (NTILE, None, None, 5), (LAG, None, column, 0, d)]
        rc, got, flags = hs_window_nav(dev, [], [], 0, items, n, n_keys=0)
        assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
        assert np.array_equal(got[0], np.concatenate([np.full(3, d), bits[:-3]]))
        assert np.array_equal(got[1], np.concatenate([bits[OB_TILE + 1:], np.full(OB_TILE + 1, d)]))
        assert np.array_equal(got[2], np.full(n, d)) and np.array_equal(got[3], np.full(n, bits[0]))
        assert np.array_equal(got[4], np.full(n, bits[-1]))  # no order key: every row a peer of every other
        assert np.array_equal(got[5], bits) and np.array_equal(got[7], bits)
        assert np.array_equal(got[6], window_nav_model(n, [], [], None, "ntile", buckets=5).astype(np.uint32))
        assert np.bincount(got[6].astype(np.int64))[1:].tolist() == [n // 5 + (b < n % 5) for b in range(5)]


def test_float_cells_come_back_bit_for_bit_nan_payloads_zeros_infinities_and_a_denormal(dev):
    """FLOATS holds two NaNs with different payloads, -0.0, +0.0, both infinities and a denormal; the default is a third
    NaN.  The ORDER key is the same FLOAT column: the peers of a NaN are NaNs of BOTH payloads, the peers of a zero zeros of
    both signs, and LAST_VALUE through the last peer still names one row's bits."""
    n = OB_TILE + 333
    rng = np.random.default_rng(12)
    column, bits = cells_of(dev, rng, n, T.FLOAT, special=True)
    assert len(set(bits.tolist())) == len(FLOATS)
    ids = rng.integers(0, 6, n)
    shape = dict(partition=[(ids, T.INTEGER)], order=[(bits.view(np.float32), T.FLOAT, True)])
    specs = [(LAG, None, 1), (LEAD, None, 1), (LAG, None, 2), (LEAD, None, 65), (FIRST_VALUE, "range", None), (LAST_VALUE, "range", None),
             (LAST_VALUE, "rows", None), (LAST_VALUE, "partition", None)]
    check_nav(dev, n, *keys_for(dev, shape, ids, bits), [(T.FLOAT, column, bits)], specs, "float specials")


def test_one_partition_across_a_round_of_the_tile_scan(dev):
    """test_gpu_window's layout: one partition starts in the first round of k_win_tiles and ends in the second."""
    n = OB_TILE * OB_TILE + 3 * OB_TILE + 5
    rng = np.random.default_rng(9)
    position = np.arange(n)
    ids = np.where(position < 1000, 0, np.where(position < n - 700, 1, 2))
    values = np.where(np.abs(position - OB_TILE * OB_TILE) < 5 * OB_TILE, 1 << 20, position // 3)
    shuffle = rng.permutation(n)
    ids, values = ids[shuffle], values[shuffle]
    typed = [(T.INTEGER, *cells_of(dev, rng, n, T.INTEGER))]
    specs = [(LEAD, None, 1), (LEAD, None, OB_TILE), (LAST_VALUE, "partition", None), (NTILE, None, 3), (LAG, None, OB_TILE)]
    cols, desc, n_part, _, _ = keys_for(dev, dict(partition=[(ids, T.INTEGER)], order=[(values, T.INTEGER, True)]), ids, values)
    check_nav(dev, n, cols, desc, n_part, [ids], [(values, True)], typed, specs, "across a round")  # the model takes the arrays


def test_the_older_items_of_a_mixed_call_are_what_the_older_entries_return(dev):
    n = SIZES[-1]
    _name, ids, values = layouts(n)[-1]
    cols, desc, n_part, part, order = keys_for(dev, shape_i32_i32(ids, values), ids, values)
    rng = np.random.default_rng(1)
    floats = (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32)
    ints = rng.integers(-999, 1000, n)
    fcol, icol = upload(dev, floats, T.FLOAT), upload(dev, ints, T.INTEGER)
    items = [(ROW_NUMBER, None, None), (LAG, None, icol, 2, 77), (DENSE_RANK, None, None), (SUM, "range", fcol), (LAST_VALUE, "range", fcol),
             (AVG, "rows", icol), (NTILE, None, None, 4), (COUNT, "partition", None)]
    rc, got, flags = hs_window_nav(dev, cols, desc, n_part, items, n)
    assert rc == 0 and flags == 0, dev._raw_lib.hs_last_error()
    rc, ranks = hs_window(dev, cols, desc, n_part, [ROW_NUMBER, DENSE_RANK], n)
    assert rc == 0
    rc, aggs, agg_flags = hs_window_agg(dev, cols, desc, n_part, [(SUM, "range", fcol), (AVG, "rows", icol), (COUNT, "partition", None)], n)
    assert rc == 0 and agg_flags == 0
    for mine, theirs in zip((got[0], got[2], got[3], got[5], got[7]), (*ranks, *aggs)):
        assert np.array_equal(mine, theirs.view(np.uint32))
    src = window_nav_model(n, part, order, np.arange(n), "lag", k=2, default=-1)
    assert np.array_equal(got[1], np.where(src >= 0, ints[np.maximum(src, 0)], 77).astype(np.int32).view(np.uint32))
    src = window_nav_model(n, part, order, np.arange(n), "last_value", frame="range")
    assert np.array_equal(got[4], floats.view(np.uint32)[src])
    assert np.array_equal(got[6], window_nav_model(n, part, order, None, "ntile", buckets=4).astype(np.uint32))


def test_refusals_are_codes_with_a_text_and_nothing_is_written(dev):
    col, stamps = upload(dev, [1, 2, 3], T.INTEGER), upload(dev, [1, 2, 3], T.TIMESTAMP)
    names = upload(dev, [b"a", b"bb", b"c"], T.STRING)
    coded = dev.dict_encode(upload(dev, [b"a", b"b", b"a"], T.STRING))
    lib = dev._raw_lib
    two = [col, col], [0, 0], 1
    rc, out, _ = hs_window_nav(dev, [col] * 13, [0] * 13, 1, [(LAG, None, col, 1, 0)], 3)
    assert rc == 2 and b"12" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, *two, [(LAG, None, col, 1, 0)] * 9, 3)
    assert rc == 2 and b"8" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (13, "rows", col, 1, 0)], 3)
    assert rc == 1 and b"function 13" in lib.hs_last_error() and untouched(out)
    for f in (FIRST_VALUE, LAST_VALUE, SUM):
        rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (f, 3, col)], 3)
        assert rc == 1 and b"item 1: frame 3" in lib.hs_last_error() and untouched(out)
    for f, bad in ((LAG, -1), (LEAD, 1 << 31), (NTILE, 0), (NTILE, 1 << 31)):
        rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (f, None, col, bad, 0)], 3)
        assert rc == 1 and b"item 1" in lib.hs_last_error() and str(bad).encode() in lib.hs_last_error() and untouched(out)
    for f in (LAG, NTILE):
        rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (f, None, col, 1, 0)], 3, no_params=True)
        assert rc == 1 and b"item 1" in lib.hs_last_error() and b"params" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (LEAD, None, col, 1, 0)], 3, no_defaults=True)
    assert rc == 1 and b"item 1" in lib.hs_last_error() and b"default" in lib.hs_last_error() and untouched(out)
    for f in (LAG, LEAD, FIRST_VALUE, LAST_VALUE):
        for value in (names, coded):  # (narrow and virtual kinds: tests/test_window_nav_cpu.py)
            rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (f, "rows", value, 1, 0)], 3)
            assert rc == 1 and b"item 1" in lib.hs_last_error() and b"HS_I32, HS_F32 or HS_I64" in lib.hs_last_error() and untouched(out)
        rc, out, _ = hs_window_nav(dev, *two, [(ROW_NUMBER, None, None), (f, "rows", None, 1, 0)], 3)   # a null column
        assert rc == 1 and b"item 1" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, *two, [(COUNT, "rows", None), (AVG, "rows", stamps)], 3)           # the aggregates' own refusal
    assert rc == 1 and b"item 1" in lib.hs_last_error() and b"HS_I32 or HS_F32" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, [col], [0], 1, [(LAG, None, col, 1, 0), (DENSE_RANK, None, None)], 3)
    assert rc == 1 and b"order key" in lib.hs_last_error() and untouched(out)
    rc, out, _ = hs_window_nav(dev, [col] * 12, [0] * 12, 11, [(LAG, None, stamps, 1, 9), (NTILE, None, None, 2), (LEAD, None, col, 0, 9)], 3)
    assert rc == 0 and out[0].tolist() == [9, 9, 9] and out[1].tolist() == [1, 1, 1] and out[2].tolist() == [1, 2, 3]
    assert out[0].dtype == np.uint64
    # and hs_window_agg still refuses function 8
    rc, _, _ = hs_window_agg(dev, *two, [(COUNT, "rows", None), (8, "rows", col)], 3)
    assert rc == 1 and b"function 8" in lib.hs_last_error()


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
EPOCH = datetime(1970, 1, 1)


def with_navigation(plain, items):
    """The model over the rows `plain` (the engine's own rows for the query without its window items): every item (name,
    function, argument name or None, partition names, [(order name, ascending)], {frame / k / default / buckets}) becomes
    one more column.  The value functions copy: the expected cell is the very Python value the engine returned."""
    out = [dict(r) for r in plain]
    for name, kind, arg, partition, order, more in items:
        column = window_nav_model(len(plain), [[r[p] for r in plain] for p in partition],
                                  [([r[o] for r in plain], ascending) for o, ascending in order],
                                  [r[arg] for r in plain] if arg else None, kind, **more)
        for r, v in zip(out, column):
            r[name] = int(v) if kind == "ntile" else v
    return out


def test_lag_and_lead_through_sql_and_the_dataframe_api(engine, api):
    C_, F = api.Col, api.F
    plain = engine.sql(f"SELECT l_shipmode, l_orderkey, l_extendedprice, l_quantity, l_shipdate FROM '{LINEITEM()}';").collect()
    spec = (["l_shipmode"], [("l_orderkey", False), ("l_extendedprice", True)])
    want = with_navigation(plain, [("prev", "lag", "l_quantity", *spec, dict(k=1, default=0.0)),
                                   ("nxt", "lead", "l_shipdate", *spec, dict(k=2, default=EPOCH))])
    over = "OVER (PARTITION BY l_shipmode ORDER BY l_orderkey DESC, l_extendedprice)"
    got = engine.sql(f"SELECT l_shipmode, l_orderkey, l_extendedprice, l_quantity, l_shipdate, LAG(l_quantity, 1, 0) {over} AS prev, "
                     f"LEAD(l_shipdate, 2, '1970-01-01') {over} AS nxt FROM '{LINEITEM()}';").collect()
    assert len(got) == 6000 and got == want
    assert all(isinstance(r["prev"], float) and isinstance(r["nxt"], datetime) for r in got)
    assert sum(r["prev"] == 0.0 for r in got) == 7 and sum(r["nxt"] == EPOCH for r in got) == 14  # one / two rows a ship mode
    keys = dict(partition_by=[C_("l_shipmode")], order_by=[C_("l_orderkey").desc(), C_("l_extendedprice")])
    frame = (api.DataFrame().table(LINEITEM())
             .select(C_("l_shipmode"), C_("l_orderkey"), C_("l_extendedprice"), C_("l_quantity"), C_("l_shipdate"))
             .window(F.lag(C_("l_quantity"), 1, 0).over(**keys).alias("prev"),
                     F.lead(C_("l_shipdate"), 2, "1970-01-01").over(**keys).alias("nxt")))
    assert frame.collect() == got


def test_first_and_last_value_under_the_default_frame_and_rows_with_ties(engine, api):
    plain = engine.sql(f"SELECT l_returnflag, l_quantity, l_orderkey FROM '{LINEITEM()}';").collect()
    spec = (["l_returnflag"], [("l_quantity", True)])
    want = with_navigation(plain, [("first", "first_value", "l_orderkey", *spec, dict(frame="range")),
                                   ("peer", "last_value", "l_orderkey", *spec, dict(frame="range")),
                                   ("own", "last_value", "l_orderkey", *spec, dict(frame="rows")),
                                   ("first_rows", "first_value", "l_orderkey", *spec, dict(frame="rows"))])
    over = "PARTITION BY l_returnflag ORDER BY l_quantity"
    got = engine.sql(f"SELECT l_returnflag, l_quantity, l_orderkey, FIRST_VALUE(l_orderkey) OVER ({over}) AS first, "
                     f"LAST_VALUE(l_orderkey) OVER ({over}) AS peer, "
                     f"LAST_VALUE(l_orderkey) OVER ({over} ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW) AS own, "
                     f"FIRST_VALUE(l_orderkey) OVER ({over} ROWS UNBOUNDED PRECEDING) AS first_rows FROM '{LINEITEM()}';").collect()
    assert got == want and all(r["own"] == r["l_orderkey"] and r["first"] == r["first_rows"] for r in got)
    assert any(r["peer"] != r["own"] for r in got)  # 50 quantities over 6000 rows: the last peer is another row nearly everywhere


def test_the_top_quarter_of_every_ship_mode(engine, api):
    plain = engine.sql(f"SELECT l_shipmode, l_orderkey, l_extendedprice FROM '{LINEITEM()}';").collect()
    bucketed = with_navigation(plain, [("q", "ntile", None, ["l_shipmode"], [("l_extendedprice", False), ("l_orderkey", True)],
                                        dict(buckets=4))])
    want = sorted((r for r in bucketed if r["q"] == 1), key=lambda r: (r["l_shipmode"], -r["l_extendedprice"], r["l_orderkey"]))
    got = engine.sql("SELECT l_shipmode, l_orderkey, l_extendedprice, NTILE(4) OVER (PARTITION BY l_shipmode ORDER BY "
                     f"l_extendedprice DESC, l_orderkey) AS q FROM '{LINEITEM()}' QUALIFY q = 1 "
                     "ORDER BY l_shipmode, l_extendedprice DESC, l_orderkey;").collect()
    assert got == want and 1500 <= len(got) <= 1507 and all(isinstance(r["q"], int) for r in got)


def test_lag_over_group_by_results(engine, api):
    plain = engine.sql(f"SELECT YEAR(l_shipdate) AS y, SUM(l_quantity) AS s FROM '{LINEITEM()}' GROUP BY y ORDER BY y;").collect()
    want = with_navigation(plain, [("prev", "lag", "s", [], [("y", True)], dict(k=1, default=0.0))])
    got = engine.sql("SELECT YEAR(l_shipdate) AS y, SUM(l_quantity) AS s, LAG(s, 1, 0) OVER (ORDER BY y) AS prev "
                     f"FROM '{LINEITEM()}' GROUP BY y ORDER BY y;").collect()
    assert got == want and len(got) > 3 and got[0]["prev"] == 0.0 and [r["prev"] for r in got[1:]] == [r["s"] for r in got[:-1]]


def test_one_spec_of_ranking_aggregate_and_navigation_items_is_one_call(engine, api, monkeypatch):
    from tests.test_gpu_window import with_windows
    from tests.test_gpu_window_agg import with_aggregates

    plain = engine.sql(f"SELECT l_shipmode, l_orderkey, l_extendedprice FROM '{LINEITEM()}';").collect()
    spec = (["l_shipmode"], [("l_orderkey", True), ("l_extendedprice", True)])
    want = with_windows(plain, [("rn", "row_number", *spec)])
    want = with_aggregates(want, [("upto", "sum", "l_orderkey", *spec, "rows")])
    want = with_navigation(want, [("prev", "lag", "l_orderkey", *spec, dict(k=1, default=-1)), ("q", "ntile", None, *spec, dict(buckets=10)),
                                  ("first", "first_value", "l_extendedprice", [], [("l_orderkey", True)], dict(frame="range"))])
    calls = []
    window = type(engine.dev).window
    monkeypatch.setattr(type(engine.dev), "window", lambda self, *a: calls.append([i.func for i in a[3]]) or window(self, *a))
    inside = "PARTITION BY l_shipmode ORDER BY l_orderkey, l_extendedprice"
    got = engine.sql(f"SELECT l_shipmode, l_orderkey, l_extendedprice, ROW_NUMBER() OVER ({inside}) AS rn, "
                     f"SUM(l_orderkey) OVER ({inside} ROWS UNBOUNDED PRECEDING) AS upto, LAG(l_orderkey, 1, -1) OVER ({inside}) AS prev, "
                     f"NTILE(10) OVER ({inside}) AS q, FIRST_VALUE(l_extendedprice) OVER (ORDER BY l_orderkey) AS first "
                     f"FROM '{LINEITEM()}';").collect()
    assert got == want
    assert sorted(calls) == [["first_value"], ["row_number", "sum", "lag", "ntile"]]  # one spec: one sort, one call


def test_a_repeated_query_returns_the_same_rows_with_replay_on(monkeypatch):
    from minispark_amd.execution import HipExecutionEngine

    monkeypatch.setenv("HIPSPARK_REPLAY", "1")
    with HipExecutionEngine(device=0) as e:
        assert e.replay_enabled
        text = ("SELECT l_shipmode, l_orderkey, LEAD(l_orderkey, 1, -1) OVER (PARTITION BY l_shipmode ORDER BY l_orderkey) AS nxt "
                f"FROM '{LINEITEM()}' QUALIFY nxt < 0;")
        runs = [e.sql(text).collect() for _ in range(3)]  # the third run would be a recorded replay without the task
    assert runs[0] == runs[1] == runs[2] and len(runs[0]) == 7


def test_a_streamed_select_with_a_navigation_item_is_refused():
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from minispark_amd.workloads import engine_api

    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: the table streams in several ranges (tests/test_gpu_streaming.py)
        api = engine_api(e)
        select = api.DataFrame().table(LINEITEM()).select(api.Col("l_orderkey"), api.Col("l_shipmode"))
        with pytest.raises(ExecutionError, match=r"OVER.*HIPSPARK_HBM_BUDGET"):
            select.window(api.F.lag(api.Col("l_orderkey"), 1, 0).over(order_by=[api.Col("l_orderkey")])).collect()


def two_rank_frame(api, paths):
    # (l_orderkey, l_extendedprice, l_quantity) orders the rows of a ship mode totally: the neighbours do not depend on
    # which rank's rows the gathered result lists first
    C_, F = api.Col, api.F
    keys = dict(partition_by=[C_("l_shipmode")], order_by=[C_("l_orderkey").desc(), C_("l_extendedprice"), C_("l_quantity")])
    return (api.DataFrame().table(paths["lineitem"])
            .select(C_("l_shipmode"), C_("l_orderkey"), C_("l_extendedprice"), C_("l_quantity"))
            .window(F.row_number().over(**keys).alias("rn"), F.lag(C_("l_quantity"), 1, -1).over(**keys).alias("prev"),
                    F.lead(C_("l_orderkey"), 2, 0).over(**keys).alias("nxt"), F.ntile(1200).over(**keys).alias("q"),
                    F.last_value(C_("l_orderkey")).over(partition_by=[C_("l_shipmode")]).alias("last"))
            .qualify(C_("rn") <= 5).order_by(C_("l_shipmode"), C_("rn")))


def test_two_ranks_navigate_the_gathered_result_on_rank_0(tmp_path, engine, api):
    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_window_nav", "two_rank_frame", "q1_multiblock", out])
    one_rank = two_rank_frame(api, load_golden("q1_multiblock")["paths"]).collect()
    got = [tuple(r) for r in json.loads(out.read_text())]
    assert got == tuples(one_rank) and len(got) == 35
    assert sum(r[5] == -1 for r in got) == 7 and all(r[4] == 1 or r[5] > 0 for r in got)
