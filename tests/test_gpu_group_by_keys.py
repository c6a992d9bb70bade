"""GROUP BY over several columns on the GPU: hs_key_pack / hs_key_unpack against a numpy byte concatenation, and the engine
against the unchanged CPU oracle - every table is written a second time with one more INTEGER column ``g``, the dense id of
the row's key tuple, and the oracle's ``GROUP BY g`` rows with ``g`` replaced by its tuple are what the engine must return,
bit for bit (FLOAT values are k/64, so every f64 sum is exact)."""

from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from datetime import datetime, timedelta
from pathlib import Path

import numpy as np
import pytest

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.io import BlockFile, StrCol
from minispark_amd.sql import Col, Functions as F
from oracle.py_engine import run_query
from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ======================================================================================================================
# kernel level
# ======================================================================================================================
PART_SETS = {"code_code": ["code", "code"], "code_x3": ["code", "code", "code"], "code_x8": ["code"] * 8, "code_i32": ["code", "i32"], "i32_i32": ["i32", "i32"], "i64_i32": ["i64", "i32"],
             "i32_str3_code_i64": ["i32", "str3", "code", "i64"]}
WIDTH = {"code": 1, "i32": 4, "i64": 8, "str3": 3}
ONE_PASS = max(hs.KEY_TILE_ROWS * hs.KEY_MAX_BLOCKS, hs.KEY_BYTES_PASS_ROWS)  # rows a single trip of either capped grid covers
ROW_COUNTS = [1, 15, 16, 17, 255, 4097, ONE_PASS + 1]  # both sides of a 16-byte vector, of a tile, of the grid's first trip


def part_values(kind: str, n: int, seed: int) -> np.ndarray:
    """rows x width bytes: negative integers, integers that differ in their top byte only, code 0 and code 255"""
    rng = np.random.default_rng(seed)
    if kind == "code":
        v = rng.integers(0, 256, n).astype(np.uint8)
        v[:: 7], v[3:: 7] = 0, 255
        return v.reshape(n, 1)
    if kind == "i32":
        v = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int64)
        v[1:: 5] = 0x00ABCDEF + ((np.arange(len(v[1:: 5])) % 256) << 24)  # equal but for the top byte (negative from 0x80 on)
        v[2:: 11] = -1
        return v.astype(np.uint32).astype("<u4").view(np.uint8).reshape(n, 4)
    if kind == "i64":
        v = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
        v[1:: 5] = 0x00123456789ABCDE + ((np.arange(len(v[1:: 5])) % 128) << 56)
        v[2:: 9] = -(1 << 63)
        return v.astype("<i8").view(np.uint8).reshape(n, 8)
    return rng.integers(32, 127, (n, 3)).astype(np.uint8)  # a fixed string of three bytes


def device_part(dev, kind: str, raw: np.ndarray):
    import torch
    from minispark_amd.device import DCol

    n = raw.shape[0]
    if kind == "i32":
        return dev.fixed_col(hs.I32, raw.reshape(-1).view(np.int32))
    if kind == "i64":
        return dev.fixed_col(hs.I64, raw.reshape(-1).view(np.int64))
    width = raw.shape[1]
    return DCol(hs.STR, dev.to_device(raw.reshape(-1), torch.uint8), n, lens=dev.const_lens(width, n), fixed_len=width)


@pytest.fixture(scope="module")
def kernel_inputs(dev):
    out = {}
    for name, kinds in PART_SETS.items():
        for n in ROW_COUNTS:
            raws = [part_values(kind, n, 100 * k + len(kinds)) for k, kind in enumerate(kinds)]
            out[name, n] = (raws, [device_part(dev, kind, raw) for kind, raw in zip(kinds, raws)])
    return out


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("name", list(PART_SETS))
def test_pack_is_the_byte_concatenation_and_unpack_its_inverse(dev, kernel_inputs, name, n):
    import torch

    kinds = PART_SETS[name]
    raws, cols = kernel_inputs[name, n]
    width = sum(WIDTH[k] for k in kinds)
    want = np.concatenate(raws, axis=1)
    assert want.shape == (n, width)
    guard = 64
    out = dev.empty(n * width + guard, torch.uint8)
    out.fill_(0xA5)
    arr = (hs.hs_col * len(cols))(*[c.as_hs() for c in cols])
    hs.check(dev.lib.hs_key_pack(dev.stream, arr, len(cols), n, out.data_ptr(), width), "hs_key_pack")
    got = out.cpu().numpy()
    assert got[: n * width].tobytes() == want.tobytes()
    assert (got[n * width:] == 0xA5).all(), "bytes behind the last row were written"

    widths = (C.c_int32 * len(kinds))(*[WIDTH[k] for k in kinds])
    n_dev = torch.tensor([n - n // 3], dtype=torch.int64, device=dev.device)  # a device-resident count below the bound
    for count, count_dev in ((n, None), (n - n // 3, n_dev)):
        outs = [dev.empty(n * WIDTH[k] + guard, torch.uint8) for k in kinds]
        for o in outs:
            o.fill_(0x5A)
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        hs.check(dev.lib.hs_key_unpack(dev.stream, out.data_ptr(), width, n, count_dev.data_ptr() if count_dev is not None else None,
                                       widths, len(outs), ptrs), "hs_key_unpack")
        for kind, raw, o in zip(kinds, raws, outs):
            back = o.cpu().numpy()
            w = WIDTH[kind]
            assert back[: count * w].tobytes() == raw[:count].tobytes(), (kind, count)
            assert (back[count * w:] == 0x5A).all(), (kind, count, "rows behind the count were written")


def test_device_pack_and_unpack_keep_kinds_and_dictionaries(dev):
    """Device.pack_key / unpack_key: the packed column is a fixed-length STRING, a code-byte part comes back coded."""
    import torch
    from minispark_amd.device import DBatch, DCol

    n = 1000
    entries = (b"AIR", b"MAIL", b"SHIP")
    codes = (np.arange(n) % 3).astype(np.uint8)
    ints = (np.arange(n, dtype=np.int64) * 7919 - 3_000_000).astype(np.int32)
    stamps = (np.arange(n, dtype=np.int64) * 86_400_000_000 - 5)
    batch = DBatch([("i", ColumnType.INTEGER), ("s", ColumnType.STRING), ("t", ColumnType.TIMESTAMP)],
                   [dev.fixed_col(hs.I32, ints),
                    DCol(hs.STR, dev.to_device(codes, torch.uint8), n, lens=dev.const_lens(1, n), fixed_len=1, dict=entries),
                    dev.fixed_col(hs.I64, stamps)], n)
    spec = dev.key_spec(batch, [1, 2, 0])
    assert spec.width == 13 and [p.name for p in spec.parts] == ["s", "t", "i"]
    packed = dev.pack_key(batch, [1, 2, 0])
    assert (packed.kind, packed.fixed_len, packed.n, packed.dict) == (hs.STR, 13, n, None)
    s, t, i = dev.unpack_key(packed, spec)
    assert (s.kind, s.fixed_len, s.dict) == (hs.STR, 1, entries) and (t.kind, i.kind) == (hs.I64, hs.I32)
    assert (s.data[:n].cpu().numpy() == codes).all() and (t.data[:n].cpu().numpy() == stamps).all()
    assert (i.data[:n].cpu().numpy() == ints).all()


# ======================================================================================================================
# engine level
# ======================================================================================================================
SIZES = {"one": [1], "two_blocks": [512, 513], "six_blocks": [1000, 1, 999, 1500, 777, 723]}  # 1, 1025 and 5000 rows
MODES = ["AIR", "MAIL", "RAIL", "SHIP"]
FLAGS = ["A", "N", "R"]
EPOCH = datetime(1995, 1, 1)
SCHEMA = [("a", ColumnType.INTEGER), ("b", ColumnType.INTEGER), ("c", ColumnType.INTEGER), ("d", ColumnType.INTEGER),
          ("s1", ColumnType.STRING), ("s2", ColumnType.STRING), ("t", ColumnType.TIMESTAMP), ("f", ColumnType.FLOAT),
          ("x", ColumnType.FLOAT), ("i", ColumnType.INTEGER), ("v", ColumnType.STRING), ("j", ColumnType.INTEGER)]
KEYS = {"int_dict": ["a", "s1"], "dict_dict": ["s1", "s2"], "int_int": ["b", "c"], "four_ints": ["a", "b", "c", "d"],
        "stamp_dict": ["t", "s2"], "refused": ["x", "v", "t"]}


def make_columns(n: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.int32)
    a = rng.integers(-1, 2, n).astype(np.int32) * 16_777_216          # three values that differ in the top byte only
    s1 = rng.integers(0, 4, n)
    s2 = rng.integers(0, 3, n)
    a[j % 97 == 5], s1[j % 97 == 5] = 7, 3                            # the tuple (7, SHIP): every row of it has i == -777
    if n > 2000:
        a[1000], s1[1000] = 99, 0                                     # the tuple (99, AIR): one row, in the one-row block
    i = rng.integers(-1000, 1000, n).astype(np.int32)
    i[j % 97 == 5] = -777
    t = np.array([int((EPOCH + timedelta(days=int(d))).timestamp() * 1_000_000) for d in rng.integers(0, 5, n)], dtype=np.int64)
    return {"a": a, "b": rng.integers(-12, 13, n).astype(np.int32), "c": rng.integers(0, 20, n).astype(np.int32),
            "d": rng.integers(0, 3, n).astype(np.int32), "s1": [MODES[k] for k in s1], "s2": [FLAGS[k] for k in s2], "t": t,
            "f": (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32),  # k/64: f64 sums are exact
            "x": (rng.integers(0, 4, n) / 64.0).astype(np.float32), "i": i,
            "v": [str(k * 37) for k in j], "j": j}  # v: thousands of distinct strings of several lengths - no dictionary


def tuple_ids(cols: dict, names: list[str]) -> tuple[np.ndarray, list[tuple]]:
    """dense id of every row's key tuple + the tuple of every id (np.unique over the rows of per-column ids)"""
    per_column, values = [], []
    for name in names:
        uniq, inverse = np.unique(np.asarray(cols[name]), return_inverse=True)
        per_column.append(inverse.astype(np.int64))
        values.append(uniq)
    rows, inverse = np.unique(np.stack(per_column, axis=1), axis=0, return_inverse=True)
    tuples = [tuple(values[k][r[k]].item() for k in range(len(names))) for r in rows]
    return inverse.reshape(-1).astype(np.int32), tuples


def write_table(path: Path, schema: list, cols: dict, sizes: list[int]) -> str:
    def blocks():
        lo = 0
        for size in sizes:
            yield [StrCol.from_strings(list(cols[c][lo: lo + size])) if t == ColumnType.STRING else np.asarray(cols[c][lo: lo + size])
                   for c, t in schema]
            lo += size

    path.parent.mkdir(parents=True, exist_ok=True)
    BlockFile(path).write_raw_blocks(list(schema), blocks())
    return str(path)


class Table:
    """One table, and per key set the same table with the INTEGER column g = the dense id of the row's key tuple."""

    def __init__(self, folder: Path, name: str, cols: dict, sizes: list[int], schema=SCHEMA, keys=KEYS) -> None:
        self.plain = write_table(folder / f"{name}.bin", schema, cols, sizes)
        self.keyed, self.tuples = {}, {}
        for key_name, names in keys.items():
            g, self.tuples[key_name] = tuple_ids(cols, names)
            self.keyed[key_name] = write_table(folder / f"{name}_{key_name}.bin", [*schema, ("g", ColumnType.INTEGER)],
                                               {**cols, "g": g}, sizes)


def as_result(value, col_type):
    return datetime.fromtimestamp(value / 1_000_000) if col_type == ColumnType.TIMESTAMP else value


def expected(table: Table, key_name: str, names: list[str], build, schema=SCHEMA) -> list[dict]:
    """The oracle's rows of ``build(frame over the g table, [Col('g')])`` with g replaced by its tuple."""
    types = dict(schema)
    rows = run_query(build(DataFrame(object()).table(table.keyed[key_name]), [Col("g")]).task)
    out = []
    for r in rows:
        tup = table.tuples[key_name][r["g"]]
        head = {name: as_result(v, types[name]) for name, v in zip(names, tup)}
        out.append({**head, **{k: v for k, v in r.items() if k != "g"}})
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    folder = tmp_path_factory.mktemp("group_by_keys")
    return {name: Table(folder, name, make_columns(sum(sizes), 70 + len(sizes)), sizes) for name, sizes in SIZES.items()}


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


AGGS = lambda: [F.sum(Col("f")).alias("sf"), F.min(Col("i")).alias("lo"), F.max(Col("f")).alias("hi"), F.count()]  # noqa: E731


def grouped(names):
    def build(frame, key=None):
        key = key if key is not None else [Col(n) for n in names]
        return frame.filter(Col("i") != -777).group_by(*key).agg(*AGGS())
    return build


@pytest.mark.parametrize("name", list(SIZES))
def test_integer_and_dictionary_string_on_the_on_chip_tier(engine, tables, name):
    names = KEYS["int_dict"]
    want = expected(tables[name], "int_dict", names, grouped(names))
    rows = grouped(names)(DataFrame(engine).table(tables[name].plain)).collect()
    assert [list(r) for r in rows[:1]] == [list(r) for r in want[:1]] and list(want[0])[:2] == names
    assert assert_rows_match(rows, want, max_ulps=0) == 0
    assert engine.dev.last_scan["tier"] in ("private", "shared")  # an LDS tier, not the HBM one
    if name == "six_blocks":
        assert len(want) == 13  # 3 x 4 tuples and (99, AIR); (7, SHIP) is dropped by the WHERE
        keys = {(r["a"], r["s1"]) for r in rows}
        assert (99, "AIR") in keys and (7, "SHIP") not in keys and {(-16_777_216, "AIR"), (0, "AIR"), (16_777_216, "AIR")} <= keys
        assert not engine._global_partial


def test_the_data_has_the_shapes_the_cases_need(tables):
    t = tables["six_blocks"]
    assert (7, "SHIP") in t.tuples["int_dict"] and (99, "AIR") in t.tuples["int_dict"]
    assert 200 < len(t.tuples["int_int"]) <= 500 and len(t.tuples["four_ints"]) > 1500


def test_a_where_that_drops_every_row_leaves_no_group(engine, tables):
    for name in SIZES:
        frame = DataFrame(engine).table(tables[name].plain).filter(Col("j") < 0).group_by(Col("a"), Col("s1")).agg(*AGGS())
        assert frame.collect() == []


SQL = ("SELECT s1, s2, COUNT() AS n, SUM(f) AS sf, AVG(i) AS m FROM '{t}' WHERE i != -777 GROUP BY ({k}) HAVING COUNT() > {c} "
       "ORDER BY s1, s2 DESC LIMIT 5;")


FLOORS = {"one": 0, "two_blocks": 82, "six_blocks": 400}  # HAVING COUNT() > floor: some tuples pass, some do not


@pytest.mark.parametrize("name", list(SIZES))
def test_two_dictionary_strings_through_sql_with_having_order_by_and_limit(engine, tables, name):
    floor = FLOORS[name]
    from minispark_amd.parser import parse_sql

    rows = run_query(parse_sql(SQL.format(t=tables[name].keyed["dict_dict"], k="g", c=floor).replace("SELECT s1, s2,", "SELECT g,")
                               .replace(" ORDER BY s1, s2 DESC LIMIT 5", ""), object()).task)
    tuples = tables[name].tuples["dict_dict"]
    want = [{"s1": tuples[r["g"]][0], "s2": tuples[r["g"]][1], **{k: v for k, v in r.items() if k != "g"}} for r in rows]
    want.sort(key=lambda r: r["s2"], reverse=True)
    want.sort(key=lambda r: r["s1"])
    want = want[:5]
    got = engine.sql(SQL.format(t=tables[name].plain, k="s1, s2", c=floor)).collect()
    assert len(want) == (5 if name != "one" else 1)
    assert [list(r) for r in got] == [list(r) for r in want]
    assert [(r["s1"], r["s2"]) for r in got] == [(r["s1"], r["s2"]) for r in want]  # in order
    for g, w in zip(got, want):
        assert assert_rows_match([g], [w], max_ulps=0) == 0


def test_two_integers_with_a_few_hundred_groups_on_the_shared_tier(engine, tables):
    names = KEYS["int_int"]
    want = expected(tables["six_blocks"], "int_int", names, grouped(names))
    assert 200 < len(want) <= 500
    frame = grouped(names)(DataFrame(engine).table(tables["six_blocks"].plain))
    assert assert_rows_match(frame.collect(), want, max_ulps=0) == 0
    assert engine.dev.last_scan["tier"] == "shared"
    assert assert_rows_match(grouped(names)(DataFrame(engine).table(tables["two_blocks"].plain)).collect(),
                             expected(tables["two_blocks"], "int_int", names, grouped(names)), max_ulps=0) == 0


def test_four_integers_with_thousands_of_groups_on_the_radix_tier(tmp_path):
    """More groups per block than the shared dictionary holds: the engine climbs to the HBM tier, where the 16-byte key
    rides the radix tier as two key words."""
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine

    constants.SHUFFLE_FOLDER = tmp_path / "shuffle"
    rng = np.random.default_rng(9)
    n, distinct = 30_000, 7_000
    pool = np.stack([rng.integers(-3, 4, distinct) * 16_777_216, rng.integers(-50, 50, distinct), rng.integers(0, 1000, distinct),
                     rng.integers(0, 2, distinct)], axis=1).astype(np.int32)
    pick = rng.integers(0, distinct, n)
    cols = {"a": pool[pick, 0], "b": pool[pick, 1], "c": pool[pick, 2], "d": pool[pick, 3],
            "f": (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32), "i": rng.integers(-1000, 1000, n).astype(np.int32)}
    schema = [("a", ColumnType.INTEGER), ("b", ColumnType.INTEGER), ("c", ColumnType.INTEGER), ("d", ColumnType.INTEGER),
              ("f", ColumnType.FLOAT), ("i", ColumnType.INTEGER)]
    table = Table(tmp_path, "wide", cols, [13_000, 1, 16_999], schema, {"four_ints": KEYS["four_ints"]})

    def build(frame, key=None):
        key = key if key is not None else [Col(c) for c in KEYS["four_ints"]]
        return frame.filter(Col("i") % 7 != 0).group_by(*key).agg(F.sum(Col("f")).alias("sf"), F.avg(Col("i")).alias("m"), F.count())

    want = expected(table, "four_ints", KEYS["four_ints"], build, schema)
    assert len(want) > 4096
    with HipExecutionEngine(0) as engine:
        frame = build(DataFrame(engine).table(table.plain))
        for _ in range(2):
            assert assert_rows_match(frame.collect(), want, max_ulps=0) == 0
        assert engine._global_partial and engine.dev.last_global_tier == "radix"


@pytest.mark.parametrize("name", list(SIZES))
def test_a_timestamp_and_a_dictionary_string_with_avg(engine, tables, name):
    names = KEYS["stamp_dict"]

    def build(frame, key=None):
        key = key if key is not None else [Col(n) for n in names]
        return frame.filter(Col("i") != -777).group_by(*key).agg(F.avg(Col("f")).alias("mf"), F.sum(Col("i")).alias("si"),
                                                                 F.avg(Col("i")).alias("mi"), F.count())

    want = expected(tables[name], "stamp_dict", names, build)
    rows = build(DataFrame(engine).table(tables[name].plain)).collect()
    assert type(rows[0]["t"]) is datetime and list(rows[0]) == ["t", "s2", "mf", "si", "mi", "count"]
    assert assert_rows_match(rows, want, max_ulps=0) == 0
    if name == "six_blocks":
        assert len(want) == 15


def test_three_runs_on_one_engine_return_the_same_rows(tables):
    """first run, recorded run, replay (where the run can be recorded)"""
    from minispark_amd.execution import HipExecutionEngine

    names = KEYS["dict_dict"]
    want = expected(tables["six_blocks"], "dict_dict", names, grouped(names))
    with HipExecutionEngine() as fresh:
        frame = grouped(names)(DataFrame(fresh).table(tables["six_blocks"].plain))
        runs = [frame.collect() for _ in range(3)]
    for rows in runs:
        assert assert_rows_match(rows, want, max_ulps=0) == 0
    order = lambda rows: sorted(rows, key=lambda r: (r["s1"], r["s2"]))  # noqa: E731 - row order is unspecified
    assert order(runs[0]) == order(runs[1]) == order(runs[2])


USERS = [("user_id", ColumnType.INTEGER), ("w", ColumnType.FLOAT), ("grp", ColumnType.INTEGER), ("region", ColumnType.STRING)]
ORDERS = [("user_id", ColumnType.INTEGER), ("price", ColumnType.FLOAT), ("quantity", ColumnType.INTEGER), ("mode", ColumnType.STRING)]


def test_a_join_feeds_a_two_column_group_by_with_keys_from_both_sides(engine, tmp_path):
    rng = np.random.default_rng(21)
    n_users, n_orders = 150, 700
    users = {"user_id": np.arange(n_users, dtype=np.int32), "w": (rng.integers(-4000, 4000, n_users) / 64.0).astype(np.float32),
             "grp": rng.integers(0, 6, n_users).astype(np.int32), "region": [FLAGS[k] for k in rng.integers(0, 3, n_users)]}
    orders = {"user_id": rng.integers(0, n_users + 40, n_orders).astype(np.int32),
              "price": (rng.integers(-4000, 4000, n_orders) / 64.0).astype(np.float32),
              "quantity": rng.integers(1, 90, n_orders).astype(np.int32), "mode": [MODES[k] for k in rng.integers(0, 4, n_orders)]}
    u_path = write_table(tmp_path / "users.bin", USERS, users, [97, 53])
    o_path = write_table(tmp_path / "orders.bin", ORDERS, orders, [300, 1, 399])
    # the oracle's side: g = the dense id of (u.grp, o.mode) cannot be a column of either table, so the pair is folded
    # into ONE INTEGER per side - gu on users, go on orders - and the joined rows are grouped by gu * 4 + go there
    go = np.array([MODES.index(m) for m in orders["mode"]], dtype=np.int32)
    u_keyed = write_table(tmp_path / "users_g.bin", [*USERS, ("gu", ColumnType.INTEGER)], {**users, "gu": users["grp"] * 4}, [97, 53])
    o_keyed = write_table(tmp_path / "orders_g.bin", [*ORDERS, ("go", ColumnType.INTEGER)], {**orders, "go": go}, [300, 1, 399])

    def aggs():
        return [F.sum(Col("o.price")).alias("sp"), F.max(Col("u.w")).alias("hw"), F.sum(Col("o.quantity")).alias("q"), F.count().alias("n")]

    def joined(eng, up, op):
        return DataFrame(eng).table(up).alias("u").join(DataFrame(eng).table(op).alias("o"), on=Col("u.user_id") == Col("o.user_id"),
                                                         how="inner")

    oracle = (joined(object(), u_keyed, o_keyed).select((Col("u.gu") + Col("o.go")).alias("g"), Col("o.price"), Col("u.w"), Col("o.quantity"))
              .group_by(Col("g")).agg(*aggs()))
    want = [{"grp": r["g"] // 4, "mode": MODES[r["g"] % 4], **{k: v for k, v in r.items() if k != "g"}} for r in run_query(oracle.task)]
    assert len(want) == 24
    frame = joined(engine, u_path, o_path).group_by(Col("u.grp"), Col("o.mode")).agg(*aggs())
    rows = frame.collect()
    assert list(rows[0]) == ["grp", "mode", "sp", "hw", "q", "n"]
    assert assert_rows_match(rows, want, max_ulps=0) == 0
    assert assert_rows_match(frame.collect(), want, max_ulps=0) == 0


def test_refusals_name_the_column_and_leave_the_engine_usable(engine, tables):
    plain = tables["six_blocks"].plain
    with pytest.raises(NotImplementedError, match='"x" is FLOAT'):
        DataFrame(engine).table(plain).group_by(Col("a"), Col("x")).agg(F.count()).collect()
    with pytest.raises(NotImplementedError, match='STRING "v"'):
        DataFrame(engine).table(plain).group_by(Col("v"), Col("a")).agg(F.count()).collect()
    with pytest.raises(NotImplementedError, match="20 bytes wide"):
        DataFrame(engine).table(plain).select(Col("t"), Col("t").alias("t2"), Col("a")).group_by(Col("t"), Col("t2"), Col("a")).agg(
            F.count()).collect()
    single = DataFrame(engine).table(plain).filter(Col("i") != -777).group_by(Col("s1")).agg(*AGGS())
    want = run_query(DataFrame(object()).table(plain).filter(Col("i") != -777).group_by(Col("s1")).agg(*AGGS()).task)
    assert assert_rows_match(single.collect(), want, max_ulps=0) == 0


# ---- the interpreter kernels, in one child process -------------------------------------------------------------------------
def hexed(rows):
    return [{k: (v.hex() if type(v) is float else str(v) if isinstance(v, datetime) else v) for k, v in r.items()} for r in rows]


def test_the_interpreter_returns_the_compiled_forms_bits(engine, tables, tmp_path):
    plain = tables["six_blocks"].plain
    names = KEYS["int_dict"]
    compiled = {"int_dict": grouped(names)(DataFrame(engine).table(plain)).collect(),
                "dict_dict": engine.sql(SQL.format(t=plain, k="s1, s2", c=FLOORS["six_blocks"])).collect()}
    out = tmp_path / "worker.json"
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "group_by_keys_worker.py"), str(out), plain],
                          env=dict(os.environ, HIPSPARK_JIT="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert proc.returncode == 0, proc.stdout.decode()[-3000:]
    got = json.loads(out.read_text())
    assert got["jit_launches"] == 0
    key = lambda r: json.dumps(r, sort_keys=True)  # noqa: E731
    assert sorted(got["int_dict"], key=key) == sorted(hexed(compiled["int_dict"]), key=key)  # floats as hex: equal bits
    assert got["dict_dict"] == hexed(compiled["dict_dict"])  # ORDER BY: in order
