"""Window ranking on the GPU.  At the C ABI (hs_window) the three columns must be EXACTLY those of the numpy definition
(tests/window_model.py): the values are integers, nothing is computed in floating point, so nothing is tolerated.  End to
end: queries over the committed golden tables, through engine.sql and the DataFrame API; the expected columns are the
model applied to the rows the same engine returns for the same query without its window items."""

from __future__ import annotations

import json

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, load_golden
from tests.ranks import run_ranks
from tests.test_gpu_count_distinct import hs_mark_first
from tests.test_gpu_distinct import _constants, hs_distinct, py_values, tuples, upload
from tests.window_abi import call_window
from tests.window_model import window_model

pytestmark = pytest.mark.gpu

_K = _constants("hs_ops.hip", "hs_radix.hip")
OB_TILE = _K["OB_TILE"]   # rows of one workgroup of the heads / scan passes
RX_TILE = _K["RX_TILE"]   # rows of one partition-pass workgroup of the sort
SIZES = [0, 1, 2, 63, 64, 65, OB_TILE - 1, OB_TILE, OB_TILE + 1, RX_TILE - 1, RX_TILE + 1, 3 * OB_TILE + RX_TILE + 17]
ROW_NUMBER, RANK, DENSE_RANK = 0, 1, 2
NAMES = {ROW_NUMBER: "row_number", RANK: "rank", DENSE_RANK: "dense_rank"}


def test_the_tile_sizes_were_found_in_the_code():
    assert (OB_TILE, RX_TILE, _K["WIN_PER"]) == (2048, 8192, 8)
    assert SIZES[-1] > 4 * OB_TILE


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def hs_window(dev, cols, descending, n_part, funcs, n, n_keys=None):
    """The entry point itself (tests/window_abi.py) -> (return code, [one int32 array per function, input order])."""
    rc, got, _ = call_window(dev, "hs_window", cols, descending, n_part, [(f,) for f in funcs], n, n_keys)
    return rc, [o.view(np.int32) for o in got]


def check(dev, partition, order, funcs=(ROW_NUMBER, RANK, DENSE_RANK), coded=()):
    """partition = [(values, type)], order = [(values, type, ascending)]: hs_window against the model, exactly.  The
    partition columns whose index is in `coded` go to the device dictionary-coded (a code byte per row)."""
    n = len((partition + order)[0][0]) if partition or order else 0
    typed = [(v, t) for v, t in partition] + [(v, t) for v, t, _ in order]
    cols = [upload(dev, v, t) for v, t in typed] if n else [upload(dev, [0], T.INTEGER) for _ in typed]
    for k in coded if n else ():  # without rows the call answers before it looks at the columns
        cols[k] = dev.dict_encode(cols[k])
        assert cols[k] is not None and cols[k].dict is not None
    want = window_model(n, [py_values(v, t) for v, t in partition], [(py_values(v, t), a) for v, t, a in order])
    desc = [0] * len(partition) + [0 if a else 1 for _, _, a in order]
    rc, got = hs_window(dev, cols, desc, len(partition), list(funcs), n)
    assert rc == 0, dev._raw_lib.hs_last_error()
    for f, column in zip(funcs, got):
        bad = np.nonzero(column != want[NAMES[f]])[0]
        assert bad.size == 0, (f"{NAMES[f]} differs at {bad.size} of {n} rows, first row {bad[0]}: got {column[bad[0]]}, "
                               f"want {want[NAMES[f]][bad[0]]}")


def layouts(n):
    """(name, partition id per row, order value per row), rows already shuffled: the sort brings the partitions together,
    so `a partition starts at sorted position p` is `p rows have a smaller id`."""
    rng = np.random.default_rng(1000 + n)
    few = lambda: rng.integers(0, max(2, int(n * 0.7)), n)  # noqa: E731 - about 30 % of the rows tie with another one
    out = [("one partition", np.zeros(n, dtype=np.int64), few()),
           ("every row its own partition", rng.permutation(n), few()),
           ("all rows peers", np.zeros(n, dtype=np.int64), np.full(n, 4))]
    if n > OB_TILE:
        out.append(("a partition starts at a tile's first row", (np.arange(n) >= OB_TILE).astype(np.int64), rng.integers(0, 9, n)))
    if n >= 4 * OB_TILE - 1:
        # 100 rows, then one partition to the end: 10 rows of it, then peers only - tiles without any head pass the carry on
        ids = (np.arange(n) >= 100).astype(np.int64)
        values = np.where(np.arange(n) < 110, np.arange(n) % 7, 9)
        out.append(("a partition over several tiles, some without a head", ids, values))
    if n:
        sizes = rng.integers(1, 201, n)
        ids = np.repeat(np.arange(n), sizes)[:n]
        out.append(("random partitions of 1 - 200 rows", ids, rng.integers(0, 140, n)))  # ~30 % ties inside a partition
    shuffled = []
    for name, ids, values in out:
        order = rng.permutation(n)
        shuffled.append((name, np.asarray(ids)[order], np.asarray(values)[order]))
    return shuffled


FLOATS = np.array([0x7fc00000, 0x80000000, 0x00000000, 0x7f800000, 0xff800000, 0x3fc00000, 0xc0100000, 0xffc00001, 0x00000001],
                  dtype=np.uint32).view(np.float32)   # NaN, -0.0, +0.0, +inf, -inf, 1.5, -2.25, another NaN, a denormal
STRINGS = [b"", b"a", b"ab", b"ab\0", b"abc", b"b", b"ab\0\0", b"abcdefghij"]


def shape_i32_i32(ids, values):
    return dict(partition=[(ids * 7 - 3, T.INTEGER)], order=[(values - 50, T.INTEGER, True)])


def shape_i32_i32_desc(ids, values):
    return dict(partition=[(ids * 7 - 3, T.INTEGER)], order=[(values - 50, T.INTEGER, False)])


def shape_timestamp_i32(ids, values):
    return dict(partition=[((ids.astype(np.int64) << 21) + (1 << 44), T.TIMESTAMP)], order=[(values, T.INTEGER, True)])


def shape_code_f32(ids, values):
    return dict(partition=[([b"p%03d" % (i % 200) for i in ids], T.STRING)], coded=(0,),
                order=[(FLOATS[values % len(FLOATS)], T.FLOAT, True)])


def shape_str12_str(ids, values):
    return dict(partition=[([b"part-%07d" % i for i in ids], T.STRING)],
                order=[([STRINGS[v % len(STRINGS)] for v in values], T.STRING, True)])


def shape_two_and_two(ids, values):
    return dict(partition=[(ids // 3, T.INTEGER), (ids % 3, T.TIMESTAMP)],
                order=[(FLOATS[(values // 2) % len(FLOATS)], T.FLOAT, False), (values % 2, T.INTEGER, True)])


def shape_no_partition(ids, values):
    return dict(partition=[], order=[(values, T.INTEGER, True)])


def shape_row_number_alone(ids, values):
    return dict(partition=[(ids, T.INTEGER)], order=[], funcs=(ROW_NUMBER,))


SHAPES = [shape_i32_i32, shape_i32_i32_desc, shape_timestamp_i32, shape_code_f32, shape_str12_str, shape_two_and_two,
          shape_no_partition, shape_row_number_alone]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda f: f.__name__[6:])
def test_every_layout_at_every_tile_boundary(dev, shape):
    for n in SIZES:
        if n == 0:
            check(dev, **shape(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
        for _name, ids, values in layouts(n):
            check(dev, **shape(ids, values))


def test_the_twelve_byte_partition_column_has_one_length(dev):
    col = upload(dev, [b"part-%07d" % i for i in range(70)], T.STRING)
    assert col.as_hs().fixed_len == 12


def test_only_the_requested_functions_are_written_in_the_order_asked(dev):
    rng = np.random.default_rng(5)
    n = OB_TILE + 300
    ids, values = rng.integers(0, 40, n), rng.integers(0, 12, n)
    check(dev, [(ids, T.INTEGER)], [(values, T.INTEGER, True)], funcs=(DENSE_RANK,))
    check(dev, [(ids, T.INTEGER)], [(values, T.INTEGER, True)], funcs=(RANK, ROW_NUMBER))
    check(dev, [(ids, T.INTEGER)], [(values, T.INTEGER, True)], funcs=(RANK, RANK, DENSE_RANK, ROW_NUMBER, ROW_NUMBER))


def test_one_partition_across_a_round_of_the_tile_scan(dev):
    """k_win_tiles takes OB_TILE summaries per round: rows beyond OB_TILE tiles lie in its second round.  One partition
    starts in the first round and ends in the second, and a long run of peers crosses the boundary with it."""
    n = OB_TILE * OB_TILE + 3 * OB_TILE + 5
    rng = np.random.default_rng(9)
    position = np.arange(n)
    ids = np.where(position < 1000, 0, np.where(position < n - 700, 1, 2))
    values = np.where(np.abs(position - OB_TILE * OB_TILE) < 5 * OB_TILE, 1 << 20, position // 3)
    order = rng.permutation(n)
    check(dev, [(ids[order], T.INTEGER)], [(values[order], T.INTEGER, True)])


RUN_KEYS = {  # n -> [(values, type)]: few values per column, so that rows repeat
    "one_word": lambda rng, n: [(rng.integers(-3, 4, n), T.INTEGER)],
    "two_words": lambda rng, n: [(rng.integers(0, 3, n), T.INTEGER), ((rng.integers(0, 3, n) << 21) + (1 << 44), T.TIMESTAMP),
                                 (rng.integers(-1, 2, n), T.INTEGER)],
    "string_and_integer": lambda rng, n: [([STRINGS[v] for v in rng.integers(0, len(STRINGS), n)], T.STRING),
                                          (rng.integers(0, 3, n), T.INTEGER)],
}


@pytest.mark.parametrize("keys", RUN_KEYS)
def test_the_three_readers_of_the_sorted_runs_see_the_same_runs(dev, keys):
    """hs_mark_first (its sort path), hs_distinct and the window entries take the sorted rows through one routine: over
    the same key columns, as ORDER BY keys of one partition, the first-occurrence marks are the rows that lead their
    peers, the surviving rows are the marked ones, and there are as many as DENSE_RANK counts.  Sizes: the wave step, the
    wave's share and the tile of the two heads kernels, and their neighbours."""
    for n in (1, 2, 64, 65, 512, 513, OB_TILE, OB_TILE + 1, 2 * OB_TILE + 1):
        columns = RUN_KEYS[keys](np.random.default_rng(2400 + n), n)
        cols = [upload(dev, v, t) for v, t in columns]
        rc, marks = hs_mark_first(dev, cols, n, mode=1)
        assert rc == 0, dev._raw_lib.hs_last_error()
        rc, (row_number, rank, dense_rank) = hs_window(dev, cols, [0] * len(cols), 0, [ROW_NUMBER, RANK, DENSE_RANK], n)
        assert rc == 0, dev._raw_lib.hs_last_error()
        rc, rows = hs_distinct(dev, cols, n)
        assert rc == 0, dev._raw_lib.hs_last_error()
        assert marks == (row_number == rank).astype(np.int32).tolist(), (keys, n)
        assert rows == np.nonzero(marks)[0].tolist(), (keys, n)
        assert len(rows) == dense_rank.max(), (keys, n)
        assert n < 64 or len(rows) < n, "rows repeat"


def test_argument_errors_are_codes_and_nothing_is_launched(dev):
    col = upload(dev, [1, 2, 3], T.INTEGER)
    lib = dev._raw_lib
    rc, out = hs_window(dev, [col] * 13, [0] * 13, 1, [ROW_NUMBER], 3)
    assert rc == 2 and b"12" in lib.hs_last_error() and out[0].tolist() == [-7] * 3
    rc, out = hs_window(dev, [col], [0], 1, [ROW_NUMBER, RANK], 3)          # a rank function without an order key
    assert rc == 1 and b"order key" in lib.hs_last_error() and out[1].tolist() == [-7] * 3
    rc, _ = hs_window(dev, [col, col], [0, 0], 1, [7], 3)
    assert rc == 1
    rc, _ = hs_window(dev, [col, col], [0, 0], 3, [ROW_NUMBER], 3)
    assert rc == 1
    rc, _ = hs_window(dev, [col, col], [0, 0], 1, [ROW_NUMBER] * 9, 3)
    assert rc == 2 and b"8" in lib.hs_last_error()
    rc, out = hs_window(dev, [col] * 12, [0] * 12, 11, [ROW_NUMBER, RANK], 3)
    assert rc == 0 and out[0].tolist() == [1, 1, 1] and out[1].tolist() == [1, 1, 1]


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


def with_windows(plain, items):
    """The model over the rows `plain` (the engine's own rows for the query without its window items): every item
    (name, function, partition names, [(order name, ascending)]) becomes one more column, behind the others."""
    out = [dict(r) for r in plain]
    for name, kind, partition, order in items:
        column = window_model(len(plain), [[r[p] for r in plain] for p in partition],
                              [([r[o] for r in plain], ascending) for o, ascending in order])[kind]
        for r, v in zip(out, column):
            r[name] = int(v)
    return out


def test_partition_by_and_order_by_desc_over_a_plain_select(engine, api):
    C, F = api.Col, api.F
    plain = lambda: api.DataFrame().table(LINEITEM()).select(C("l_shipmode"), C("l_orderkey"), C("l_quantity"))  # noqa: E731
    want = with_windows(plain().collect(), [("rn", "row_number", ["l_shipmode"], [("l_quantity", False)]),
                                            ("rk", "rank", ["l_shipmode"], [("l_quantity", False)]),
                                            ("dr", "dense_rank", ["l_shipmode"], [("l_quantity", False)])])
    over = "OVER (PARTITION BY l_shipmode ORDER BY l_quantity DESC)"
    got = engine.sql(f"SELECT l_shipmode, l_orderkey, l_quantity, ROW_NUMBER() {over} AS rn, RANK() {over} AS rk, "
                     f"DENSE_RANK() {over} AS dr FROM '{LINEITEM()}';").collect()
    assert len(got) == 6000 and got == want
    assert max(r["rn"] for r in got) > 700 and any(r["rk"] != r["rn"] for r in got) and any(r["dr"] != r["rk"] for r in got)
    spec = dict(partition_by=[C("l_shipmode")], order_by=[C("l_quantity").desc()])
    frame = plain().window(F.row_number().over(**spec).alias("rn"), F.rank().over(**spec).alias("rk"),
                           F.dense_rank().over(**spec).alias("dr"))
    assert frame.collect() == got


def test_a_window_over_a_group_by_result(engine, api):
    text = ("SELECT l_shipmode, l_returnflag, COUNT() AS n, RANK() OVER (PARTITION BY l_shipmode ORDER BY n DESC) AS r, "
            f"DENSE_RANK() OVER (ORDER BY l_shipmode DESC) AS d FROM '{LINEITEM()}' GROUP BY (l_shipmode, l_returnflag);")
    plain = engine.sql(f"SELECT l_shipmode, l_returnflag, COUNT() AS n FROM '{LINEITEM()}' GROUP BY (l_shipmode, l_returnflag);").collect()
    want = with_windows(plain, [("r", "rank", ["l_shipmode"], [("n", False)]), ("d", "dense_rank", [], [("l_shipmode", False)])])
    got = engine.sql(text).collect()
    # RANK and DENSE_RANK do not depend on the order the grouped rows come in
    assert sorted(tuples(got)) == sorted(tuples(want)) and len(got) == len(plain) > 7
    assert list(got[0]) == ["l_shipmode", "l_returnflag", "n", "r", "d"] and {r["d"] for r in got} == set(range(1, 8))


def test_a_window_over_the_rows_of_a_join(engine, api):
    g = load_golden("e2e_join_select")
    C, F = api.Col, api.F
    joined = lambda: (api.DataFrame().table(g["paths"]["users"]).alias("u")  # noqa: E731
                      .join(api.DataFrame().table(g["paths"]["orders"]).alias("o"), on=C("u.user_id") == C("o.user_id"), how="inner")
                      .select(C("u.country"), C("o.product"), C("o.price")))
    want = with_windows(joined().collect(), [("rn", "row_number", ["country"], [("price", False), ("product", True)])])
    got = joined().window(F.row_number().over(partition_by=[C("u.country")], order_by=[C("o.price").desc(), C("o.product")])
                          .alias("rn")).collect()
    assert got == want and list(got[0]) == ["country", "product", "price", "rn"] and max(r["rn"] for r in got) > 1
    text = ("SELECT u.country, o.product, o.price, ROW_NUMBER() OVER (PARTITION BY u.country ORDER BY o.price DESC, o.product) AS rn "
            f"FROM '{g['paths']['users']}' AS u JOIN '{g['paths']['orders']}' AS o ON u.user_id=o.user_id;")
    assert engine.sql(text).collect() == got


def test_the_top_three_of_every_group(engine, api):
    plain = engine.sql(f"SELECT l_shipmode AS k, l_orderkey, l_extendedprice FROM '{LINEITEM()}';").collect()
    ranked = with_windows(plain, [("rn", "row_number", ["k"], [("l_extendedprice", False)])])
    want = sorted((r for r in ranked if r["rn"] <= 3), key=lambda r: (r["k"], r["rn"]))
    got = engine.sql("SELECT l_shipmode AS k, l_orderkey, l_extendedprice, ROW_NUMBER() OVER (PARTITION BY k ORDER BY "
                     f"l_extendedprice DESC) AS rn FROM '{LINEITEM()}' QUALIFY rn <= 3 ORDER BY k, rn;").collect()
    assert got == want and len(got) == 21


def test_qualify_with_distinct_and_limit(engine, api):
    plain = engine.sql(f"SELECT l_shipmode, l_returnflag FROM '{LINEITEM()}';").collect()
    ranked = with_windows(plain, [("d", "dense_rank", [], [("l_shipmode", True)])])
    kept = list(dict.fromkeys(tuples(r for r in ranked if r["d"] > 2)))       # QUALIFY, then DISTINCT ...
    want = sorted(kept, key=lambda r: (-r[2], r[1]))[:4]                       # ... then ORDER BY and LIMIT
    got = engine.sql("SELECT DISTINCT l_shipmode, l_returnflag, DENSE_RANK() OVER (ORDER BY l_shipmode) AS d "
                     f"FROM '{LINEITEM()}' QUALIFY d > 2 ORDER BY d DESC, l_returnflag LIMIT 4;").collect()
    assert tuples(got) == want and len(got) == 4
    C, F = api.Col, api.F
    frame = (api.DataFrame().table(LINEITEM()).select(C("l_shipmode"), C("l_returnflag"))
             .window(F.dense_rank().over(order_by=[C("l_shipmode")]).alias("d")).qualify(C("d") > 2).distinct()
             .order_by(C("d").desc(), C("l_returnflag")).limit(4))
    assert frame.collect() == got


def test_two_items_share_a_spec_and_one_has_another_in_the_middle_of_the_select_list(engine, api, monkeypatch):
    plain = engine.sql(f"SELECT l_returnflag, l_orderkey, l_quantity FROM '{LINEITEM()}';").collect()
    want = with_windows(plain, [("a", "rank", ["l_returnflag"], [("l_quantity", True)]),
                                ("b", "dense_rank", ["l_returnflag"], [("l_quantity", True)]),
                                ("row_number", "row_number", [], [("l_orderkey", False)])])
    calls = []
    window = type(engine.dev).window
    monkeypatch.setattr(type(engine.dev), "window", lambda self, *a: calls.append([i.func for i in a[3]]) or window(self, *a))
    got = engine.sql("SELECT l_returnflag, RANK() OVER (PARTITION BY l_returnflag ORDER BY l_quantity) AS a, l_orderkey, "
                     "ROW_NUMBER() OVER (ORDER BY l_orderkey DESC), DENSE_RANK() OVER (PARTITION BY l_returnflag ORDER BY "
                     f"l_quantity ASC) AS b, l_quantity FROM '{LINEITEM()}';").collect()
    assert list(got[0]) == ["l_returnflag", "a", "l_orderkey", "row_number", "b", "l_quantity"]  # the select list's order
    assert [{k: r[k] for k in want[0]} for r in got] == want
    assert sorted(calls) == [["rank", "dense_rank"], ["row_number"]]  # one sort per spec


def test_a_repeated_windowed_query_returns_the_same_rows_with_replay_on(monkeypatch):
    from minispark_amd.execution import HipExecutionEngine

    monkeypatch.setenv("HIPSPARK_REPLAY", "1")
    with HipExecutionEngine(device=0) as e:
        assert e.replay_enabled
        text = (f"SELECT l_shipmode, l_orderkey, ROW_NUMBER() OVER (PARTITION BY l_shipmode ORDER BY l_orderkey) AS rn "
                f"FROM '{LINEITEM()}' QUALIFY rn <= 2;")
        runs = [e.sql(text).collect() for _ in range(3)]  # the third run would be a recorded replay without the task
    assert runs[0] == runs[1] == runs[2] and len(runs[0]) == 14


def test_a_streamed_select_with_a_window_is_refused():
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from minispark_amd.workloads import engine_api

    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: the table streams in several ranges (tests/test_gpu_streaming.py)
        api = engine_api(e)
        select = api.DataFrame().table(LINEITEM()).select(api.Col("l_orderkey"), api.Col("l_shipmode"))
        with pytest.raises(ExecutionError, match=r"OVER.*HIPSPARK_HBM_BUDGET"):
            select.window(api.F.row_number().over(order_by=[api.Col("l_orderkey")])).collect()


def two_rank_frame(api, paths):
    # (l_orderkey, l_extendedprice, l_quantity) orders the rows of a ship mode totally: ROW_NUMBER does not depend on
    # which rank's rows the gathered result lists first
    C, F = api.Col, api.F
    keys = dict(partition_by=[C("l_shipmode")], order_by=[C("l_orderkey").desc(), C("l_extendedprice"), C("l_quantity")])
    return (api.DataFrame().table(paths["lineitem"])
            .select(C("l_shipmode"), C("l_orderkey"), C("l_extendedprice"), C("l_quantity"))
            .window(F.row_number().over(**keys).alias("rn"), F.dense_rank().over(**keys).alias("dr"))
            .qualify(C("rn") <= 5).order_by(C("l_shipmode"), C("rn")))


def test_two_ranks_rank_the_gathered_result_on_rank_0(tmp_path, engine, api):
    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_window", "two_rank_frame", "q1_multiblock", out])
    one_rank = two_rank_frame(api, load_golden("q1_multiblock")["paths"]).collect()
    got = [tuple(r) for r in json.loads(out.read_text())]
    assert got == tuples(one_rank) and len(got) == 35
