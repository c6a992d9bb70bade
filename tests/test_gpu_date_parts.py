"""Date parts and DATE_TRUNC on the GPU: HS_OP_DATEPART through hs_eval in both evaluator forms against the integer model
of tests/date_part_model.py, bit for bit, over the calendar's edge cells and the whole i64 range; then engine.sql(...) / the
DataFrame API / the native scan stage against the oracle extended by that model - every comparison bit-exact (timestamps
are whole seconds between 1900 and 2096, so ``datetime`` round-trips; FLOAT values are k/64, so every f64 sum is exact)."""

from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.io import BlockFile
from minispark_amd.parser import parse_sql
from minispark_amd.sql import Col, Functions as F, Lit
from oracle.py_engine import run_query
from tests import date_part_model as model
from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
US_PER_DAY = 86_400_000_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ======================================================================================================================
# kernel level: hs_eval through the C ABI
# ======================================================================================================================
@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


def word(op, sp, a=0, b=0, c=0):
    return op | (sp << 8) | (a << 16) | (b << 32) | (c << 48)


def raw_program(words, lits=()):
    p = hs.hs_program()
    p.n_ins, p.n_lit = len(words), len(lits)
    for i, w in enumerate(words):
        p.ins[i] = w
    for i, w in enumerate(lits):
        p.lit[i] = w & 0xFFFFFFFFFFFFFFFF
    return p


def at(*args) -> int:
    return model.to_cell(datetime(*args))


def around(cell: int) -> list[int]:
    return [cell - 1, cell, cell + 1]


ERA_STARTS = [(-719_468 + k * 146_097) * US_PER_DAY for k in range(2, 8)]  # 1970 lies in era 4: two eras to either side
EDGE_CELLS = list(dict.fromkeys([  # (2000-03-01 is also an era's first day: once)
    *around(0), *around(US_PER_DAY), *around(-US_PER_DAY),
    at(2000, 2, 29), at(2000, 3, 1), at(1900, 2, 28), at(1900, 3, 1), at(2100, 2, 28), at(2100, 3, 1), at(2024, 2, 29),
    at(2023, 12, 31, 23, 59, 59, 999999), at(2024, 1, 1),
    *[c for month in (1, 4, 7, 10) for c in (at(2023, month, 1) - 1, at(2023, month, 1))],
    at(2024, 3, 3, 23, 59, 59, 999999), at(2024, 3, 4),  # a Sunday's last microsecond, the Monday after
    -719_468 * US_PER_DAY - 1, -719_468 * US_PER_DAY,     # 0000-03-01 and the microsecond before it
    *[c for start in ERA_STARTS for c in around(start)],
    at(1, 1, 1), at(9999, 12, 31), at(9999, 12, 31, 23, 59, 59, 999999),
    I64_MIN + 1, I64_MAX - 1, I64_MIN, I64_MAX,
]))
ROW_COUNTS = [1, 3, 4, 5, 255, 1023, 1025, 4099]
LD, LIT, DP, OUT = hs.OP_LD, hs.OP_LIT, hs.OP_DATEPART, hs.OP_OUT
PART_SELECTORS, TRUNC_SELECTORS = list(range(9)), list(range(16, 24))


def cells_for(n: int) -> np.ndarray:
    """The edge cells, padded with seeded random cells over the whole i64 range, cycled to n rows; fewer rows than edge
    cells take the END of the list (the extremes)."""
    rng = np.random.default_rng(1970)
    pad = rng.integers(I64_MIN, I64_MAX, max(ROW_COUNTS), dtype=np.int64, endpoint=True)
    base = np.concatenate([np.array(EDGE_CELLS, dtype=np.int64), pad])
    return base[:n].copy() if n >= len(EDGE_CELLS) else np.array(EDGE_CELLS[-n:], dtype=np.int64)


def other_cells(n: int) -> np.ndarray:
    return (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)


# column slots: 0 t (the cells), 1 x, 2 y (cells that must be left alone).  name -> (program, expected cells of OUT k)
def _each(selectors):
    words = []
    for k, sel in enumerate(selectors):
        words += [word(LD, 0, 0), word(DP, 1, sel), word(OUT, 1, k)]
    return raw_program(words)


PROGRAMS = {
    # the opcode at stack depth 1, once per selector
    "parts_at_sp1": (_each(PART_SELECTORS), lambda t, x, y: [model.part(s, t) for s in PART_SELECTORS]),
    "truncations_at_sp1": (_each(TRUNC_SELECTORS), lambda t, x, y: [model.part(s, t) for s in TRUNC_SELECTORS]),
    # seven cells below the operand: DATEPART at sp = HS_MAX_STACK rewrites cell 7 and leaves cells 0 .. 6 alone
    "part_at_max_stack": (raw_program([word(LD, 0, 1), word(LD, 1, 2), word(LD, 2, 0), word(LD, 3, 2), word(LD, 4, 1), word(LD, 5, 0),
                                       word(LD, 6, 2), word(LD, 7, 0), word(DP, 8, 8),
                                       *[word(OUT, 8 - k, k) for k in range(8)]]),
                          lambda t, x, y: [model.part(8, t), y, t, x, y, t, y, x]),
    "truncation_at_max_stack": (raw_program([word(LD, 0, 1), word(LD, 1, 2), word(LD, 2, 0), word(LD, 3, 2), word(LD, 4, 1),
                                             word(LD, 5, 0), word(LD, 6, 2), word(LD, 7, 0), word(DP, 8, 19),
                                             *[word(OUT, 8 - k, k) for k in range(8)]]),
                                lambda t, x, y: [model.part(19, t), y, t, x, y, t, y, x]),
    # a truncation feeds a part (and another truncation); a literal operand
    "truncation_feeds_part": (raw_program([word(LD, 0, 0), word(DP, 1, 17), word(DP, 1, 2), word(OUT, 1, 0),
                                           word(LD, 0, 0), word(DP, 1, 19), word(DP, 1, 7), word(OUT, 1, 1),
                                           word(LD, 0, 0), word(DP, 1, 18), word(DP, 1, 16), word(DP, 1, 8), word(OUT, 1, 2),
                                           word(LIT, 0, 0), word(DP, 1, 0), word(LD, 1, 0), word(DP, 2, 3), word(hs.OP_ADD_I, 2),
                                           word(OUT, 1, 3)], [at(2024, 2, 29, 12)]),
                              lambda t, x, y: [model.part(2, model.part(17, t)), model.part(7, model.part(19, t)),
                                               model.part(8, model.part(16, model.part(18, t))), 2024 + model.part(3, t)]),
}


@pytest.fixture(scope="module")
def kernel_inputs(dev):
    """host columns and their device copies per row count, uploaded once"""
    out = {}
    for n in ROW_COUNTS:
        t = cells_for(n)
        host = [t, other_cells(n), np.roll(t, 1) ^ np.int64(-1)]
        out[n] = (host, [dev.fixed_col(hs.I64, np.ascontiguousarray(h, dtype=np.int64)) for h in host])
    return out


def test_the_edge_cells_cover_what_they_name():
    cells = np.array(EDGE_CELLS, dtype=np.int64)
    assert len(set(EDGE_CELLS)) == len(EDGE_CELLS) == 54 and len(EDGE_CELLS) < 255
    assert model.civil_from_days(-719_468) == (0, 3, 1) and model.part(7, at(2024, 3, 3)) == 7 and model.part(7, at(2024, 3, 4)) == 1
    years = model.part(0, cells)
    assert {0, 1, 1900, 2000, 2100, 9999, -290308, 294247} <= set(years.tolist())
    assert [model.civil_from_days(s // US_PER_DAY) for s in ERA_STARTS] == [(y, 3, 1) for y in (800, 1200, 1600, 2000, 2400, 2800)]
    assert cells_for(1).tolist() == [I64_MAX] and cells_for(5).tolist() == EDGE_CELLS[-5:] and len(cells_for(4099)) == 4099


@pytest.mark.parametrize("jit", [1, 0], ids=["compiled", "interpreter"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_every_selector_equals_the_model_in_both_evaluator_forms(dev, kernel_inputs, n, jit):
    import torch

    host, cols = kernel_inputs[n]
    arr = (hs.hs_col * len(cols))(*[c.as_hs() for c in cols])
    stats = (C.c_int32 * 3)()
    dev.lib.hs_jit_stats(stats)
    launched, failed = stats[1], stats[2]
    dev.reset_flags()
    dev.lib.hs_jit_set_enabled(jit)
    try:
        for name, (prog, expect) in PROGRAMS.items():
            want = expect(*host)
            outs = [dev.empty(n, torch.int64) for _ in want]
            for o in outs:
                o.fill_(0x5A5A5A5A5A5A5A5A)
            ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            kinds = (C.c_int32 * len(outs))(*[hs.I64] * len(outs))
            hs.check(dev.lib.hs_eval(dev.stream, arr, len(cols), C.byref(prog), None, n, None, ptrs, kinds, len(outs),
                                     dev.flags.data_ptr()), "hs_eval")
            for k, (o, w) in enumerate(zip(outs, want)):
                got = o.cpu().numpy()
                w = np.asarray(w, dtype=np.int64)
                bad = np.nonzero(got != w)[0]
                assert got.tobytes() == w.tobytes(), (name, k, n, jit, [(int(host[0][i]), int(got[i]), int(w[i])) for i in bad[:5]])
        assert dev.read_flags() == 0  # the functions raise nothing; HS_FLAG_BAD_PROGRAM here = the opcode is unknown
        dev.lib.hs_jit_stats(stats)
        assert stats[2] == failed, dev.lib.hs_jit_last_log()
        assert (stats[1] - launched == len(PROGRAMS)) if jit else (stats[1] == launched), "not the evaluator form asked for"
    finally:
        dev.lib.hs_jit_set_enabled(1)
        dev.reset_flags()


@pytest.mark.parametrize("jit", [1, 0], ids=["compiled", "interpreter"])
@pytest.mark.parametrize("selector", [9, 15, 24, 0xFFFF])
def test_a_selector_out_of_range_is_a_bad_program(dev, kernel_inputs, selector, jit):
    """The generator declines it (tests/test_date_parts_cpu.py), the interpreter that takes the program then reports it."""
    import torch

    n = 255
    _, cols = kernel_inputs[n]
    arr = (hs.hs_col * len(cols))(*[c.as_hs() for c in cols])
    prog = raw_program([word(LD, 0, 0), word(DP, 1, selector), word(OUT, 1, 0)])
    out = dev.empty(n, torch.int64)
    dev.reset_flags()
    dev.lib.hs_jit_set_enabled(jit)
    try:
        ptrs, kinds = (C.c_void_p * 1)(out.data_ptr()), (C.c_int32 * 1)(hs.I64)
        hs.check(dev.lib.hs_eval(dev.stream, arr, len(cols), C.byref(prog), None, n, None, ptrs, kinds, 1, dev.flags.data_ptr()), "hs_eval")
        assert dev.read_flags() == hs.FLAG_BAD_PROGRAM
    finally:
        dev.lib.hs_jit_set_enabled(1)
        dev.reset_flags()


def test_programs_with_every_selector_compile():
    """hs_jit_compile_check / _scalar / _eval: the translator covers DATEPART (the interpreter fallback would make every
    parity test pass while the hot path is not the new one)."""
    from tests.test_date_parts_cpu import check_datepart_programs_compile

    check_datepart_programs_compile()


# ======================================================================================================================
# engine level
# ======================================================================================================================
SCHEMA = [("d", ColumnType.TIMESTAMP), ("x", ColumnType.FLOAT), ("k", ColumnType.INTEGER), ("j", ColumnType.INTEGER)]
SIZES = [1000, 1, 999, 1500, 777, 723]  # 5000 rows in six ragged blocks
SPECIAL = [(1996, 2, 29), (2000, 2, 29), (1900, 2, 28), (1900, 3, 1), (2024, 2, 29, 23, 59, 59), (1969, 12, 31, 23, 59, 59),
           (1970, 1, 1), (1995, 12, 31, 23, 59, 59), (1996, 1, 1), (2096, 1, 1), (1900, 1, 1), (2024, 3, 3, 23, 59, 59), (2024, 3, 4)]


def make_columns(n: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    lo, hi = at(1900, 1, 1) // 1_000_000, at(2096, 1, 1) // 1_000_000
    seconds = rng.integers(lo, hi, n)
    near = rng.integers(at(1994, 1, 1) // 1_000_000, at(1998, 1, 1) // 1_000_000, n)  # half the rows: five years, so groups repeat
    seconds = np.where(rng.random(n) < 0.5, near, seconds)
    for i, stamp in enumerate(SPECIAL):
        seconds[(i * 397 + 11) % n] = at(*stamp) // 1_000_000
    return {"d": (seconds * 1_000_000).astype(np.int64), "x": (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32),
            "k": rng.integers(0, 4, n).astype(np.int32), "j": np.arange(n, dtype=np.int32)}


def write_table(path: Path, cols: dict, sizes: list[int]) -> str:
    def blocks():
        lo = 0
        for size in sizes:
            yield [np.asarray(cols[c][lo: lo + size]) for c, _ in SCHEMA]
            lo += size

    BlockFile(path).write_raw_blocks(list(SCHEMA), blocks())
    return str(path)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return write_table(tmp_path_factory.mktemp("date_parts") / "t.bin", make_columns(sum(SIZES), 19), SIZES)


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


def T(eng, path):
    return DataFrame(eng).table(path)


SELECT_SQL = ("SELECT j, YEAR(d) AS y, QUARTER(d) AS q, MONTH(d) AS m, DAY(d) AS dd, HOUR(d) AS h, MINUTE(d) AS mi, SECOND(d) AS s, "
              "DAYOFWEEK(d) AS dow, DAYOFYEAR(d) AS doy, YEAR(d) * 100 + MONTH(d) AS ym, DATE_TRUNC('week', d) AS w, "
              "DATE_TRUNC('quarter', d) AS tq, YEAR(DATE_TRUNC('quarter', d)) AS yq FROM '{t}';")
WHERE_SQL = "SELECT j, d FROM '{t}' WHERE MONTH(d) = 2 AND DAY(d) = 29;"
WHERE_TRUNC_SQL = "SELECT j, d FROM '{t}' WHERE DATE_TRUNC('year', d) >= '1996-01-01' AND DATE_TRUNC('month', d) < '1996-03-01';"
CASE_GROUPED_SQL = ("SELECT k, SUM(CASE WHEN YEAR(d) = 1996 THEN x ELSE 0 END) AS x96, SUM(DAYOFWEEK(d)) AS dows, "
                    "MAX(DAYOFYEAR(d)) AS last, COUNT() AS n FROM '{t}' GROUP BY k;")
CASE_KEYLESS_SQL = ("SELECT SUM(CASE WHEN YEAR(d) = 1996 THEN x ELSE 0 END) AS x96, MIN(YEAR(d)) AS first, MAX(HOUR(d) * 60 + MINUTE(d)) AS late, "
                    "COUNT() AS n FROM '{t}' WHERE DAYOFWEEK(d) != 7;")
ALIAS_SQL = "SELECT YEAR(d) AS y, SUM(x) AS sx, COUNT() AS n FROM '{t}' WHERE j != 3 GROUP BY y ORDER BY y;"
TRUNC_KEY_SQL = "SELECT DATE_TRUNC('month', d) AS m, SUM(x) AS sx, COUNT() AS n FROM '{t}' GROUP BY m ORDER BY m;"
PLAIN_QUERIES = {"select": SELECT_SQL, "where": WHERE_SQL, "where_trunc": WHERE_TRUNC_SQL, "case_grouped": CASE_GROUPED_SQL}


def model_rows(text: str) -> list[dict]:
    """The oracle's rows for a text (no ORDER BY: the oracle has none), with the model installed for the computation only."""
    mp = pytest.MonkeyPatch()
    try:
        model.install(mp)
        return run_query(parse_sql(text, object()).task)
    finally:
        mp.undo()


def model_frame_rows(frame) -> list[dict]:
    mp = pytest.MonkeyPatch()
    try:
        model.install(mp)
        return run_query(frame.task)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def wanted(table):
    out = {name: model_rows(text.format(t=table)) for name, text in PLAIN_QUERIES.items()}
    out["alias"] = model_rows(ALIAS_SQL.format(t=table).replace(" ORDER BY y", ""))
    out["trunc_key"] = model_rows(TRUNC_KEY_SQL.format(t=table).replace(" ORDER BY m", ""))
    return out


@pytest.mark.parametrize("query", list(PLAIN_QUERIES))
def test_sql_against_the_model(engine, table, wanted, query):
    rows = engine.sql(PLAIN_QUERIES[query].format(t=table)).collect()
    want = wanted[query]
    assert [list(r) for r in rows[:1]] == [list(r) for r in want[:1]]
    assert assert_rows_match(rows, want) == 0  # max_ulps = 0: equal bits
    if query == "select":
        assert len(want) == sum(SIZES) and type(rows[0]["w"]) is datetime and type(rows[0]["y"]) is int
    if query == "where":
        assert {1996, 2000, 2024} <= {r["d"].year for r in want} and all((r["d"].month, r["d"].day) == (2, 29) for r in want)
    if query == "where_trunc":
        assert 20 < len(want) < 500 and all((r["d"].year, r["d"].month) in ((1996, 1), (1996, 2)) for r in want)
    if query == "case_grouped":
        assert sorted(r["k"] for r in want) == [0, 1, 2, 3] and all(r["x96"] != 0.0 for r in want)


def test_keyless_aggregates_over_parts(engine, table):
    """The keyless kernel (hs_agg_scalar) against the same aggregates grouped by a constant column in the oracle."""
    rows = engine.sql(CASE_KEYLESS_SQL.format(t=table)).collect()
    assert engine.dev.last_scan["tier"] == "scalar"
    d, x = Col("d"), Col("x")
    grouped = (T(object(), table).filter(F.dayofweek(d) != 7).select((Col("k") * 0).alias("g"), d, x).group_by(Col("g")).agg(
        F.sum(F.when(F.year(d) == 1996, x).otherwise(0)).alias("x96"), F.min(F.year(d)).alias("first"),
        F.max(F.hour(d) * 60 + F.minute(d)).alias("late"), F.count().alias("n")))
    want = [{k: v for k, v in r.items() if k != "g"} for r in model_frame_rows(grouped)]
    assert len(rows) == 1 and want[0]["first"] == 1900 and assert_rows_match(rows, want) == 0


def test_group_by_year_through_the_api_and_the_alias_text(engine, table, wanted):
    want = wanted["alias"]
    assert len(want) > 100 and sum(r["n"] for r in want) == sum(SIZES) - 1
    api = (T(engine, table).filter(Col("j") != 3).select(F.year(Col("d")).alias("y"), Col("x")).group_by(Col("y"))
           .agg(F.sum(Col("x")).alias("sx"), F.count().alias("n")).select(Col("y"), Col("sx"), Col("n")))
    assert assert_rows_match(api.collect(), want) == 0
    rows = engine.sql(ALIAS_SQL.format(t=table)).collect()
    assert rows == sorted(want, key=lambda r: r["y"])  # ORDER BY y: the years are unique, the order is total


def test_group_by_two_projected_parts_through_the_key_tuple(engine, table):
    d = Col("d")

    def frame(eng):
        return (T(eng, table).select(F.year(d).alias("y"), F.month(d).alias("m"), Col("x"), Col("k")).filter(Col("k") != 2)
                .group_by(Col("y"), Col("m")).agg(F.sum(Col("x")).alias("sx"), F.count().alias("n")))

    one_key = (T(object(), table).select((F.year(d) * 100 + F.month(d)).alias("g"), Col("x"), Col("k")).filter(Col("k") != 2)
               .group_by(Col("g")).agg(F.sum(Col("x")).alias("sx"), F.count().alias("n")))
    want = [{"y": r["g"] // 100, "m": r["g"] % 100, "sx": r["sx"], "n": r["n"]} for r in model_frame_rows(one_key)]
    rows = frame(engine).collect()
    assert len(want) > 150 and list(rows[0]) == ["y", "m", "sx", "n"]
    assert assert_rows_match(rows, want) == 0
    text = f"SELECT YEAR(d) AS y, MONTH(d) AS m, SUM(x) AS sx, COUNT() AS n FROM '{table}' WHERE k != 2 GROUP BY (y, m);"
    assert assert_rows_match(engine.sql(text).collect(), want) == 0


def test_group_by_a_truncation_with_order_by(engine, table, wanted):
    want = wanted["trunc_key"]
    assert len(want) > 150 and all(type(r["m"]) is datetime and r["m"].day == 1 and r["m"].hour == 0 for r in want)
    rows = engine.sql(TRUNC_KEY_SQL.format(t=table)).collect()
    assert rows == sorted(want, key=lambda r: r["m"])
    api = (T(engine, table).select(F.date_trunc("month", Col("d")).alias("m"), Col("x")).group_by(Col("m"))
           .agg(F.sum(Col("x")).alias("sx"), F.count().alias("n")))
    assert assert_rows_match(api.collect(), want) == 0


def test_the_native_scan_stage_groups_by_a_year_key(engine, table):
    from minispark_amd.stage import NativeEngine, NativeStage, lower_stage_plan

    def frame(eng):
        d = Col("d")
        return (T(eng, table).select(F.year(d).alias("y"), Col("x"), Col("j"), d).filter(Col("j") != 5).group_by(Col("y"))
                .agg(F.sum(Col("x")).alias("sx"), F.sum(F.when(F.month(d) == 2, 1).otherwise(0)).alias("feb"), F.max(F.dayofyear(d)).alias("last"),
                     F.count().alias("n")))

    assert lower_stage_plan(frame(object()).task)[0].key_computed == 1
    want = model_frame_rows(frame(object()))
    from_engine = frame(engine).collect()
    assert assert_rows_match(from_engine, want) == 0
    with NativeEngine(0) as native:
        stage = NativeStage(native, frame(object()).task)
        for _ in range(3):  # first run, recorded run, a replay
            assert assert_rows_match(stage.run(), want) == 0
        stage.close()


# ---- refusals: the error, and nothing launched ----------------------------------------------------------------------------
class CountingLib:
    """Every call into the library by name (the checks below raise before the first one)."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self._calls.append(name)
            return fn(*args)

        return call


REFUSALS = [
    (lambda eng, t: T(eng, t).select(F.year(Col("k")).alias("y")), TypeError, "YEAR\\(k\\)"),
    (lambda eng, t: T(eng, t).select(F.date_trunc("month", Col("x")).alias("m")), TypeError, "DATE_TRUNC\\('month', x\\)"),
    (lambda eng, t: T(eng, t).filter(F.month(Lit("1995-01-01")) == 1).select(Col("j")), TypeError, "MONTH\\(1995-01-01\\)"),
    (lambda eng, t: T(eng, t).group_by(Col("k")).agg(F.sum(F.dayofweek(Col("j") + 1)).alias("s")), TypeError, "DAYOFWEEK"),
    (lambda eng, t: T(eng, t).agg(F.max(F.year(Col("x"))).alias("s")), TypeError, "YEAR\\(x\\)"),
    (lambda eng, t: T(eng, t).group_by(Col("k")).agg(F.max(F.date_trunc("day", Col("d"))).alias("s")), AssertionError, "numeric"),
    (lambda eng, t: engine_sql(eng, f"SELECT YEAR('1995-01-01') AS y FROM '{t}';"), TypeError, "YEAR"),
    (lambda eng, t: engine_sql(eng, f"SELECT DATE_TRUNC('fortnight', d) AS y FROM '{t}';"), ValueError, "DATE_TRUNC unit"),
]


def engine_sql(eng, text):
    return eng.sql(text)


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_raise_before_any_launch(engine, table, monkeypatch, case):
    build, error, match = REFUSALS[case]
    calls: list[str] = []
    monkeypatch.setattr(engine.dev, "lib", CountingLib(engine.dev.lib, calls))
    monkeypatch.setattr(engine.dev, "_raw_lib", CountingLib(engine.dev._raw_lib, calls))
    with pytest.raises(error, match=match):
        build(engine, table).collect()
    quiet = ("bytes", "geom", "stats", "error", "version")
    assert [name for name in calls if not any(word in name for word in quiet)] == []


# ---- the other evaluator form, in one child process -----------------------------------------------------------------------
def hexed(rows):
    return [{k: (v.hex() if type(v) is float else str(v) if type(v) is datetime else v) for k, v in r.items()} for r in rows]


WORKER_QUERIES = {"case_grouped": CASE_GROUPED_SQL, "keyless": CASE_KEYLESS_SQL, "alias": ALIAS_SQL, "trunc_key": TRUNC_KEY_SQL,
                  "where": WHERE_SQL}


def test_the_interpreter_returns_the_compiled_forms_bits(engine, table, tmp_path):
    stats = (C.c_int32 * 3)()
    engine.dev._raw_lib.hs_jit_stats(stats)
    before, failed = stats[1], stats[2]
    compiled = {name: hexed(engine.sql(text.format(t=table)).collect()) for name, text in WORKER_QUERIES.items()}
    engine.dev._raw_lib.hs_jit_stats(stats)
    assert stats[1] > before and stats[2] == failed, "the compiled form did not run in this process"
    out = tmp_path / "worker.json"
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "date_parts_worker.py"), str(out), table],
                          env=dict(os.environ, HIPSPARK_JIT="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert proc.returncode == 0, proc.stdout.decode()[-3000:]
    got = json.loads(out.read_text())
    assert got["jit_launches"] == 0
    key = lambda r: json.dumps(r, sort_keys=True)  # noqa: E731
    for name in WORKER_QUERIES:
        assert sorted(got[name], key=key) == sorted(compiled[name], key=key), name  # floats as hex: equal bits
