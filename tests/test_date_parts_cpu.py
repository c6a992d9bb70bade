"""Date parts and DATE_TRUNC without a GPU: the integer model of tests/date_part_model.py against two independent
calendars (numpy's datetime64, Python's datetime), the grammar against the API, the exact programs the lowering emits
(HS_OP_DATEPART), the stage lowering's bounds, the generated kernels compiled for gfx950 - and one guard that holds before
the feature too: expressions without the new nodes keep the program bytes they had
(tests/golden/date_parts_parent.json, recorded from the commit before the functions existed)."""

from __future__ import annotations

import ctypes as C
import json
from datetime import datetime, timedelta
from pathlib import Path

import numpy as np
import pytest

import oracle.py_engine as py_engine
from minispark_amd import hipspark as hs
from minispark_amd import sql as sql_module
from minispark_amd import tasks as t
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.lowering import ProgramBuilder, expr_key, lower_aggregate
from minispark_amd.parser import SemanticError, parse_sql
from minispark_amd.sql import Col, DatePartColumn, DateTruncColumn, Functions as F, Lit
from tests import date_part_model as model

PARENT = json.loads((Path(__file__).parent / "golden" / "date_parts_parent.json").read_text())
SCHEMA = [(n, getattr(ColumnType, ty)) for n, ty in PARENT["schema"]]  # a b INTEGER, f FLOAT, s d STRING, ts t2 TIMESTAMP
KINDS = list(PARENT["kinds"])
DICTS = [None if d is None else tuple(e.encode() for e in d) for d in PARENT["dicts"]]
PART_FUNCTIONS = {"year": F.year, "quarter": F.quarter, "month": F.month, "day": F.day, "hour": F.hour, "minute": F.minute,
                  "second": F.second, "dayofweek": F.dayofweek, "dayofyear": F.dayofyear}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
US_PER_DAY = 86_400_000_000


# ---- the model against independent calendars ---------------------------------------------------------------------------
def numpy_fields(cells: np.ndarray) -> dict:
    """The parts of int64 microsecond cells by numpy's datetime64 unit conversions (which floor) - no formula of the model."""
    us = cells.view("datetime64[us]")
    days, months, years = us.astype("datetime64[D]"), us.astype("datetime64[M]"), us.astype("datetime64[Y]")
    month = months.astype(np.int64) - years.astype("datetime64[M]").astype(np.int64) + 1
    weekday = np.zeros(len(cells), dtype=np.int64)
    for iso, mask in enumerate(("Mon", "Tue", "Wed", "Thu", "Fri", "Sat", "Sun"), start=1):
        weekday[np.is_busday(days, weekmask=mask)] = iso
    return {
        "year": years.astype(np.int64) + 1970, "quarter": (month - 1) // 3 + 1, "month": month,
        "day": (days - months.astype("datetime64[D]")).astype(np.int64) + 1,
        "hour": (us.astype("datetime64[h]") - days.astype("datetime64[h]")).astype(np.int64),
        "minute": (us.astype("datetime64[m]") - us.astype("datetime64[h]").astype("datetime64[m]")).astype(np.int64),
        "second": (us.astype("datetime64[s]") - us.astype("datetime64[m]").astype("datetime64[s]")).astype(np.int64),
        "dayofweek": weekday, "dayofyear": (days - years.astype("datetime64[D]")).astype(np.int64) + 1,
    }


def numpy_truncations(cells: np.ndarray, fields: dict) -> dict:
    us = cells.view("datetime64[us]")
    out = {unit: us.astype(f"datetime64[{code}]").astype("datetime64[us]").astype(np.int64)
           for unit, code in (("year", "Y"), ("month", "M"), ("day", "D"), ("hour", "h"), ("minute", "m"), ("second", "s"))}
    months = us.astype("datetime64[M]")
    out["quarter"] = (months - (fields["month"] - 1) % 3).astype("datetime64[us]").astype(np.int64)
    out["week"] = (us.astype("datetime64[D]") - (fields["dayofweek"] - 1)).astype("datetime64[us]").astype(np.int64)
    return out


def assert_model_equals_numpy(cells: np.ndarray, truncations: bool = True) -> None:
    fields = numpy_fields(cells)
    for sel, name in enumerate(model.PARTS):
        np.testing.assert_array_equal(model.part(sel, cells), fields[name], err_msg=name)
    if truncations:
        want = numpy_truncations(cells, fields)
        for k, unit in enumerate(model.UNITS):
            np.testing.assert_array_equal(model.part(model.TRUNC_BASE + k, cells), want[unit], err_msg=unit)


def test_every_day_of_the_years_1_to_9999_against_numpy():
    first = int(np.datetime64("0001-01-01", "D").astype(np.int64))
    last = int(np.datetime64("9999-12-31", "D").astype(np.int64))
    days = np.arange(first, last + 1, dtype=np.int64)
    assert len(days) == 3_652_059 and model.civil_from_days(first) == (1, 1, 1) and model.civil_from_days(last) == (9999, 12, 31)
    time_of_day = (days * 7_919_000_123) % US_PER_DAY  # every day at another microsecond of the day
    time_of_day[::5] = 0
    time_of_day[1::5] = US_PER_DAY - 1
    assert_model_equals_numpy(days * US_PER_DAY + time_of_day)


def test_random_cells_against_datetime():
    rng = np.random.default_rng(20261019)
    lo, hi = model.to_cell(datetime(1, 1, 1)), model.to_cell(datetime(9999, 12, 31, 23, 59, 59, 999999))
    cells = rng.integers(lo, hi + 1, 120_000)
    cells[:4] = [lo, hi, 0, -1]
    stamps = [model.from_cell(c) for c in cells.tolist()]
    want = {"year": [d.year for d in stamps], "quarter": [(d.month - 1) // 3 + 1 for d in stamps], "month": [d.month for d in stamps],
            "day": [d.day for d in stamps], "hour": [d.hour for d in stamps], "minute": [d.minute for d in stamps],
            "second": [d.second for d in stamps], "dayofweek": [d.isoweekday() for d in stamps],
            "dayofyear": [d.timetuple().tm_yday for d in stamps]}
    for sel, name in enumerate(model.PARTS):
        assert model.part(sel, cells).tolist() == want[name], name
    trunc = {"year": lambda d: d.replace(month=1, day=1, hour=0, minute=0, second=0, microsecond=0),
             "quarter": lambda d: d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1, hour=0, minute=0, second=0, microsecond=0),
             "month": lambda d: d.replace(day=1, hour=0, minute=0, second=0, microsecond=0),
             "week": lambda d: (d - timedelta(days=d.isoweekday() - 1)).replace(hour=0, minute=0, second=0, microsecond=0)
             if d >= datetime(1, 1, 8) else None,
             "day": lambda d: d.replace(hour=0, minute=0, second=0, microsecond=0),
             "hour": lambda d: d.replace(minute=0, second=0, microsecond=0),
             "minute": lambda d: d.replace(second=0, microsecond=0), "second": lambda d: d.replace(microsecond=0)}
    for k, unit in enumerate(model.UNITS):
        got = model.part(model.TRUNC_BASE + k, cells).tolist()
        for g, d in zip(got, stamps):
            w = trunc[unit](d)
            assert w is None or g == model.to_cell(w), (unit, d)
    # the scalar form (Python integers) is the array form, cell by cell
    for sel in [*range(9), *range(16, 24)]:
        assert [model.part(sel, c) for c in cells[:2000].tolist()] == model.part(sel, cells[:2000]).tolist()


def test_beyond_datetime_down_to_the_i64_extremes_against_numpy():
    rng = np.random.default_rng(7)
    cells = rng.integers(I64_MIN + 1, I64_MAX, 200_000, dtype=np.int64, endpoint=True)
    # numpy's own unit conversions overflow inside the first day of the range (they subtract before they divide), and
    # I64_MIN itself is its NaT: the array comparison starts one day in, the first day is read from numpy's ISO rendering
    cells[:2] = [I64_MIN + US_PER_DAY, I64_MAX]
    cells = cells[cells >= I64_MIN + US_PER_DAY]
    assert_model_equals_numpy(cells, truncations=False)
    inner = cells[np.abs(cells // US_PER_DAY) < 106_751_991 - 366]  # the unit's first microsecond is representable
    assert len(inner) > 190_000
    assert_model_equals_numpy(inner)
    first_day = [I64_MIN + 1, I64_MIN + 2, I64_MIN + 1_000_000, I64_MIN + 14_454_775_808, I64_MIN + 14_454_775_807,
                 I64_MIN + US_PER_DAY - 1, *rng.integers(I64_MIN + 1, I64_MIN + US_PER_DAY, 2000).tolist()]
    for cell in first_day:
        text = str(np.int64(cell).view("datetime64[us]"))  # -290308-12-21T19:59:05.224193
        date, clock = text.split("T")
        year, month, day = date[1:].split("-")
        hour, minute, second = clock.split(":")
        want = [-int(year), (int(month) + 2) // 3, int(month), int(day), int(hour), int(minute), int(second.split(".")[0])]
        assert [model.part(sel, cell) for sel in range(7)] == want, text
    assert str(np.int64(I64_MIN + 1).view("datetime64[us]")) == "-290308-12-21T19:59:05.224193"
    monday = np.is_busday(np.int64(I64_MIN + US_PER_DAY).view("datetime64[us]").astype("datetime64[D]"), weekmask="Mon")
    assert monday and model.part(7, I64_MIN + US_PER_DAY) == 1  # so the first day is a Sunday, the 356th of its year
    assert [model.part(sel, I64_MIN) for sel in range(9)] == [-290308, 4, 12, 21, 19, 59, 5, 7, 356]
    assert [model.part(sel, I64_MIN + 1) for sel in range(9)] == [model.part(sel, I64_MIN) for sel in range(9)]
    assert str(np.int64(I64_MAX).view("datetime64[us]")) == "294247-01-10T04:00:54.775807"
    assert [model.part(sel, I64_MAX) for sel in range(9)] == [294247, 1, 1, 10, 4, 0, 54, 7, 10]


def test_floor_division_before_the_epoch():
    assert [model.part(sel, -1) for sel in (0, 2, 3, 4, 5, 6, 7, 8)] == [1969, 12, 31, 23, 59, 59, 3, 365]
    assert [model.part(sel, 0) for sel in (0, 1, 2, 3, 4, 5, 6, 7, 8)] == [1970, 1, 1, 1, 0, 0, 0, 4, 1]  # a Thursday
    assert model.part(20, -1) == -US_PER_DAY and model.part(23, -1) == -1_000_000 and model.part(16, -1) == -365 * US_PER_DAY
    assert model.part(19, 0) == -3 * US_PER_DAY  # Monday 1969-12-29


def test_truncation_wraps_only_in_front_of_the_first_representable_microsecond():
    """Total over i64, no flag: every unit that holds INT64_MIN (-290308-12-21T19:59:05.224192) starts before it, so its first
    microsecond is not representable and the result wraps; one day later the day and the shorter units are exact."""
    exact_day = (I64_MIN // US_PER_DAY) * US_PER_DAY
    assert exact_day < I64_MIN and model.part(20, I64_MIN) == exact_day + (1 << 64) > 0
    for sel in range(16, 24):
        assert model.part(sel, I64_MIN) > 0
    for sel, unit_us in ((20, US_PER_DAY), (21, 3_600_000_000), (22, 60_000_000), (23, 1_000_000)):
        cell = I64_MIN + US_PER_DAY
        assert cell - unit_us < model.part(sel, cell) <= cell and model.part(sel, cell) % unit_us == 0
    for sel in range(16, 24):
        assert 0 <= I64_MAX - model.part(sel, I64_MAX) < 366 * US_PER_DAY


def test_the_selector_tables_agree():
    assert hs.DATE_PARTS == sql_module.DATE_PARTS == model.PARTS and hs.DATE_TRUNC_UNITS == sql_module.DATE_TRUNC_UNITS == model.UNITS
    assert hs.OP_DATEPART == 38 and hs.DATE_TRUNC_BASE == model.TRUNC_BASE == 16
    assert sorted(PART_FUNCTIONS) == sorted(hs.DATE_PARTS)


# ---- nodes -------------------------------------------------------------------------------------------------------------
def test_the_nodes():
    y = F.year(Col("l_shipdate"))
    assert type(y) is DatePartColumn and y.name == "year_l_shipdate" and str(y) == "YEAR(l_shipdate)" and y.part == "year"
    m = F.date_trunc("month", Col("l_shipdate"))
    assert type(m) is DateTruncColumn and m.name == "date_trunc_month_l_shipdate" and m.unit == "month"
    assert str(m) == "DATE_TRUNC('month', l_shipdate)" and F.date_trunc("MONTH", Col("l_shipdate")).unit == "month"
    assert y.infer_type(SCHEMA[:0] + [("l_shipdate", ColumnType.TIMESTAMP)]) == ColumnType.INTEGER
    assert m.infer_type([("l_shipdate", ColumnType.TIMESTAMP)]) == ColumnType.TIMESTAMP
    assert F.year(m).infer_type([("l_shipdate", ColumnType.TIMESTAMP)]) == ColumnType.INTEGER
    assert F.year(Lit(datetime(2024, 2, 29))).infer_type([]) == ColumnType.INTEGER
    assert [c.name for c in F.year(m).all_nested_columns if type(c) is Col] == ["l_shipdate"]
    assert hash(F.year(Col("d"))) == hash(F.year(Col("d"))) != hash(F.month(Col("d")))
    assert hash(F.date_trunc("day", Col("d"))) != hash(F.date_trunc("hour", Col("d")))
    assert expr_key(F.year(Col("d"))) == ("datepart", "year", ("col", "d")) != expr_key(F.month(Col("d")))
    assert expr_key(F.date_trunc("week", Col("d"))) == ("datetrunc", "week", ("col", "d"))
    assert str(F.year(F.max(Col("d"))).normalize_agg_columns()) == "YEAR(max_d)"
    assert str(F.date_trunc("day", F.max(Col("d"))).normalize_agg_columns()) == "DATE_TRUNC('day', max_d)"


@pytest.mark.parametrize("unit", ["fortnight", "", "years", "dayofweek", 3, None])
def test_a_bad_unit_is_a_value_error_when_the_node_is_built(unit):
    with pytest.raises(ValueError, match="DATE_TRUNC unit"):
        F.date_trunc(unit, Col("d"))
    with pytest.raises(ValueError, match="date part"):
        DatePartColumn("week", Col("d"))


@pytest.mark.parametrize("arg,word", [(Col("a"), "INTEGER"), (Col("f"), "FLOAT"), (Col("s"), "STRING"), (Lit("1995-01-01"), "STRING"),
                                      (Col("a") + 1, "INTEGER"), (F.year(Col("ts")), "INTEGER")])
def test_the_argument_must_be_a_timestamp(arg, word):
    for node in (F.year(arg), F.date_trunc("month", arg), F.dayofweek(F.date_trunc("day", arg))):
        with pytest.raises(TypeError, match=word) as err:
            node.infer_type(SCHEMA)
        assert "(" in str(err.value) and str(arg) in str(err.value)  # names the expression
        b = ProgramBuilder(SCHEMA, KINDS, DICTS)
        with pytest.raises(TypeError, match=word) as err:
            b.emit_out(0, node)
        assert str(arg) in str(err.value) and b.ins == []  # raised before anything is emitted


# ---- parser ------------------------------------------------------------------------------------------------------------
_MIRROR = {"lt": "gt", "le": "ge", "gt": "lt", "ge": "le", "eq": "eq", "ne": "ne"}


def canon(col) -> str:
    """One rendering per expression, whichever way Python built it (``literal <op> column`` turned around), that walks
    into CASE and into the date functions."""
    kind = type(col).__name__
    if kind == "BinaryOperatorColumn":
        left, right, op = col.left_side, col.right_side, col.operator.__name__
        if op in _MIRROR and type(left).__name__ == "Lit" and type(right).__name__ != "Lit":
            left, right, op = right, left, _MIRROR[op]
        return f"({canon(left)} {op} {canon(right)})"
    if kind == "AliasColumn":
        return f"{canon(col.original_col)} AS {col.name}"
    if kind == "AggCol":
        return f"{col.type}({canon(col.original_col)}) AS {col.name}"
    if kind == "CaseColumn":
        return f"CASE({canon(col.condition)} ? {canon(col.then_col)} : {canon(col.else_col)})"
    if kind == "DatePartColumn":
        return f"{col.part.upper()}({canon(col.original_col)})"
    if kind == "DateTruncColumn":
        return f"DATE_TRUNC({col.unit!r}, {canon(col.original_col)})"
    return str(col)


def render(task) -> list[str]:
    out, node = [], task
    while node is not None and type(node).__name__ != "VoidTask":
        name = type(node).__name__
        if name == "FilterTask":
            out.append(f"Filter({canon(node.condition)})")
        elif name == "ProjectTask":
            out.append("Project(" + ", ".join(canon(c) for c in node.columns) + ")")
        elif name == "AggregateTask":
            out.append(f"Aggregate({node.group_by_column}; " + ", ".join(canon(c) for c in node.agg_columns) + ")")
        else:
            out.append(node.describe())
        node = node.parent_task
    return out


def T(name="t"):
    return DataFrame(object()).table(name)


def call(name: str, arg=None):
    arg = Col("d") if arg is None else arg
    return F.date_trunc("month", arg) if name == "date_trunc" else PART_FUNCTIONS[name](arg)


def text_of(name: str, arg: str = "d") -> str:
    return f"DATE_TRUNC('month', {arg})" if name == "date_trunc" else f"{name.upper()}({arg})"


NAMES = [*hs.DATE_PARTS, "date_trunc"]


@pytest.mark.parametrize("name", NAMES)
def test_every_function_builds_the_tree_of_the_api_wherever_it_may_stand(name):
    fn, api = text_of(name), call(name)
    bound = "'1995-01-01'" if name == "date_trunc" else "3"
    api_bound = "1995-01-01" if name == "date_trunc" else Lit(3)
    cases = [
        (f"SELECT {fn} AS x, a FROM 't';", T().select(api.alias("x"), Col("a"))),
        (f"SELECT a FROM 't' WHERE {fn} >= {bound} AND a > 1;", T().filter((api >= api_bound) & (Col("a") > 1)).select(Col("a"))),
        (f"SELECT CASE WHEN {fn} = {bound} THEN a ELSE 0 END AS x FROM 't';",
         T().select(F.when(api == api_bound, Col("a")).otherwise(0).alias("x"))),
        (f"SELECT YEAR(DATE_TRUNC('quarter', d)) AS y, {text_of(name, 'DATE_TRUNC(' + chr(39) + 'week' + chr(39) + ', d)')} AS x FROM 't';",
         T().select(F.year(F.date_trunc("quarter", Col("d"))).alias("y"), call(name, F.date_trunc("week", Col("d"))).alias("x"))),
    ]
    if name != "date_trunc":  # an INTEGER: an aggregate's argument, arithmetic, a CASE branch
        cases += [
            (f"SELECT k, SUM({fn}) AS s, MAX({fn} * 2 + 1) AS m FROM 't' GROUP BY k;",
             T().group_by(Col("k")).agg(F.sum(api).alias("s"), F.max(api * 2 + 1).alias("m")).select(Col("k"), Col("s"), Col("m"))),
            (f"SELECT SUM(CASE WHEN a > 1 THEN {fn} ELSE 0 END) AS s FROM 't';",
             T().agg(F.sum(F.when(Col("a") > 1, api).otherwise(0)).alias("s"))),
        ]
    for sql, want in cases:
        got = parse_sql(sql, object()).task
        assert render(got) == render(want.task), sql
        assert text_of(name).split("(")[0] in "".join(render(got))


def test_nested_calls_keep_their_classes():
    col = parse_sql("SELECT YEAR(DATE_TRUNC('quarter', d)) AS y FROM 't';", object()).task.columns[0].original_col
    assert type(col) is DatePartColumn and type(col.original_col) is DateTruncColumn and col.original_col.unit == "quarter"
    assert col.name == "year_date_trunc_quarter_d"


ALIAS_SQL = "SELECT YEAR(l_shipdate) AS y, SUM(l_quantity) AS q FROM 'lineitem' GROUP BY y ORDER BY y;"


def test_group_by_on_the_alias_of_a_date_function_builds_the_dataframe_idiom():
    ship = Col("l_shipdate")
    want = (T("lineitem").select(F.year(ship).alias("y"), Col("l_quantity")).group_by(Col("y")).agg(F.sum(Col("l_quantity")).alias("q"))
            .select(Col("y"), Col("q")).order_by(Col("y")))
    got = parse_sql(ALIAS_SQL, object()).task
    assert render(got) == render(want.task)
    assert [type(n).__name__ for n in got.task_chain] == ["LoadTableBlockTask", "ProjectTask", "AggregateTask", "ProjectTask", "SortTask"]
    # the row form with a second, plain key; HAVING's aggregate reads a column no select item names
    row = parse_sql("SELECT DATE_TRUNC('month', d) AS m, k, SUM(a * b) AS s FROM 't' GROUP BY (m, k) HAVING SUM(c) > 3;", object()).task
    want = (T().select(F.date_trunc("month", Col("d")).alias("m"), Col("k"), Col("a"), Col("b"), Col("c")).group_by(Col("m"), Col("k"))
            .agg(F.sum(Col("a") * Col("b")).alias("s"), F.sum(Col("c")).alias("_having_sum_c")).filter(Col("_having_sum_c") > 3)
            .select(Col("m"), Col("k"), Col("s")))
    assert render(row) == render(want.task)
    assert type(row.parent_task.parent_task.group_by_column).__name__ == "KeyTupleCol"
    # the plain key first, the row form with one name, the bare form
    for text in ("SELECT k, YEAR(d) AS y, COUNT() AS n FROM 't' GROUP BY (k, y);", "SELECT YEAR(d) AS y, COUNT() AS n FROM 't' GROUP BY (y);"):
        chain = [type(n).__name__ for n in parse_sql(text, object()).task.task_chain]
        assert chain == ["LoadTableBlockTask", "ProjectTask", "AggregateTask", "ProjectTask"]
    assert render(parse_sql("SELECT k, YEAR(d) AS y, COUNT() AS n FROM 't' GROUP BY (k, y);", object()).task)[-2] == "Project(k, YEAR(d) AS y)"


def test_the_alias_rule_is_limited_to_date_function_items():
    from minispark_amd.parser import GroupByError

    plain = parse_sql("SELECT k AS y, SUM(a) AS s FROM 't' GROUP BY y;", object()).task  # parsed before: keeps its tree
    assert [type(n).__name__ for n in plain.task_chain] == ["LoadTableBlockTask", "AggregateTask", "ProjectTask"]
    with pytest.raises(GroupByError):  # a date function that is no key is a stray item, as any expression is
        parse_sql("SELECT k, YEAR(d) AS y, SUM(a) AS s FROM 't' GROUP BY k;", object())
    with pytest.raises(ValueError, match="date function"):
        parse_sql("SELECT YEAR(d) AS y, SUM(y) AS s FROM 't' GROUP BY y;", object())


def test_any_other_function_name_is_still_a_semantic_error():
    for text in ("SELECT a FROM 't' WHERE UPPER(a) = 'X';", "SELECT year(d) AS y FROM 't';", "SELECT WEEK(d) AS y FROM 't';",
                 "SELECT EXTRACT(d) AS y FROM 't';", "SELECT Date_Trunc('day', d) AS y FROM 't';"):
        with pytest.raises(SemanticError):
            parse_sql(text, object())


def test_a_bad_unit_or_argument_count_in_a_text():
    with pytest.raises(ValueError, match="DATE_TRUNC unit"):
        parse_sql("SELECT DATE_TRUNC('fortnight', d) AS y FROM 't';", object())
    with pytest.raises(ValueError, match="DATE_TRUNC unit"):
        parse_sql("SELECT DATE_TRUNC(d, 'month') AS y FROM 't';", object())
    for text in ("SELECT YEAR(d, e) AS y FROM 't';", "SELECT YEAR() AS y FROM 't';", "SELECT DATE_TRUNC('month') AS y FROM 't';"):
        with pytest.raises(AssertionError, match="argument"):
            parse_sql(text, object())


# ---- lowering ------------------------------------------------------------------------------------------------------------
def ins(program) -> list[tuple]:
    return [(w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xffff, (w >> 32) & 0xffff, (w >> 48) & 0xffff) for w in program.ins]


def lower_out(expr):
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    tag = b.emit_out(0, expr)
    return tag, b.finish()


@pytest.mark.parametrize("sel,name", list(enumerate(hs.DATE_PARTS)))
def test_a_part_is_the_operand_then_one_instruction(sel, name):
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    assert b.value_tag(PART_FUNCTIONS[name](Col("ts"))) == "I"
    tag, p = lower_out(PART_FUNCTIONS[name](Col("ts")))
    assert tag == "I" and p.columns == [5] and p.max_depth == 1 and p.lits == []
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_DATEPART, 1, sel, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]


@pytest.mark.parametrize("k,unit", list(enumerate(hs.DATE_TRUNC_UNITS)))
def test_a_truncation_is_timestamp_valued(k, unit):
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    assert b.value_tag(F.date_trunc(unit, Col("ts"))) == "T"
    tag, p = lower_out(F.date_trunc(unit, Col("ts")))
    assert tag == "T" and ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_DATEPART, 1, 16 + k, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]


def test_nesting_arithmetic_and_a_literal_argument():
    tag, p = lower_out(F.year(F.date_trunc("quarter", Col("t2"))) * 100 + F.month(Col("ts")))
    assert tag == "I" and p.columns == [6, 5] and p.lits == [100] and p.max_depth == 2
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_DATEPART, 1, 17, 0, 0), (hs.OP_DATEPART, 1, 0, 0, 0), (hs.OP_LIT, 1, 0, 0, 0),
                      (hs.OP_MUL_I, 2, 0, 0, 0), (hs.OP_LD, 1, 1, 0, 0), (hs.OP_DATEPART, 2, 2, 0, 0), (hs.OP_ADD_I, 2, 0, 0, 0),
                      (hs.OP_OUT, 1, 0, 0, 0)]
    tag, p = lower_out(F.dayofyear(Lit(datetime(2024, 12, 31))) + Col("a"))
    assert tag == "I" and p.lits == [model.to_cell(datetime(2024, 12, 31))] and ins(p)[:2] == [(hs.OP_LIT, 0, 0, 0, 0), (hs.OP_DATEPART, 1, 8, 0, 0)]
    tag, p = lower_out(F.hour(Col("ts")) / 2)  # an INTEGER like any other: converted for the true division
    assert tag == "F" and [i[0] for i in ins(p)] == [hs.OP_LD, hs.OP_DATEPART, hs.OP_LIT, hs.OP_I2F, hs.OP_I2F, hs.OP_DIV_F, hs.OP_OUT]


def test_a_string_literal_next_to_a_truncation_is_a_timestamp():
    tag, p = lower_out(F.date_trunc("month", Col("ts")) >= "1995-01-01")
    assert tag == "B" and p.lits == [model.to_cell(datetime(1995, 1, 1))]
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_DATEPART, 1, 18, 0, 0), (hs.OP_LIT, 1, 0, 0, 0), (hs.OP_GE_I, 2, 0, 0, 0),
                      (hs.OP_OUT, 1, 0, 0, 0)]
    tag, p = lower_out(Lit("1995-01-01") < F.date_trunc("day", Col("ts")))  # on either side
    assert tag == "B" and p.lits == [model.to_cell(datetime(1995, 1, 1))]
    assert lower_out(F.date_trunc("day", Col("ts")) == Col("t2"))[0] == "B"
    cond = F.date_trunc("month", Col("ts")) >= "1995-01-01"
    assert cond.infer_type(SCHEMA) == ColumnType.TIMESTAMP and type(cond.right_side.value) is datetime  # as next to a column
    with pytest.raises(TypeError, match="Type mismatch"):
        lower_out(F.year(Col("ts")) >= "1995-01-01")  # a part is an INTEGER: no rewrite
    with pytest.raises(TypeError, match="Type mismatch"):
        lower_out(F.date_trunc("day", Col("ts")) > Col("a"))


def test_where_aggregate_arguments_and_the_refusal_of_a_truncation_as_one():
    leap_day = (F.month(Col("ts")) == 2) & (F.day(Col("ts")) == 29)
    low = lower_aggregate(SCHEMA, KINDS, [leap_day], Col("a"),
                          [F.sum(F.when(F.year(Col("ts")) == 1996, Col("f")).otherwise(0)), F.max(F.dayofweek(Col("ts"))),
                           F.max(F.dayofweek(Col("ts"))), F.sum(F.year(Col("ts")))], DICTS)
    assert low.acc_ops == [hs.AGG_SUM, hs.AGG_MAX, hs.AGG_SUM] and low.acc_is_int == [False, True, True] and low.agg_to_acc == [0, 1, 1, 2]
    ops = [i[0] for i in ins(low.program)]
    assert ops.count(hs.OP_DATEPART) == 5 and ops.index(hs.OP_FILTER) < ops.index(hs.OP_KEY) < ops.index(hs.OP_AGG)
    keyless = lower_aggregate(SCHEMA, KINDS, [], None, [F.sum(F.year(Col("ts")))], DICTS)
    assert keyless.key_slot == -1 and [i[0] for i in ins(keyless.program)] == [hs.OP_LD, hs.OP_DATEPART, hs.OP_AGG]
    with pytest.raises(AssertionError, match="aggregate argument must be numeric"):
        lower_aggregate(SCHEMA, KINDS, [], Col("a"), [F.max(F.date_trunc("day", Col("ts")))], DICTS)
    with pytest.raises(ValueError, match="GroupBy"):  # a computed key is projected first
        lower_aggregate(SCHEMA, KINDS, [], F.year(Col("ts")), [F.sum(Col("a"))], DICTS)
    with pytest.raises(TypeError, match="CASE branches"):
        lower_out(F.when(Col("a") > 1, F.date_trunc("day", Col("ts"))).otherwise(Col("ts")))


@pytest.mark.parametrize("name", sorted(PARENT["exprs"]))
def test_programs_without_the_nodes_keep_the_bytes_of_the_parent(name):
    _, p = lower_out(eval(PARENT["exprs"][name], {"Col": Col, "Lit": Lit, "F": F}))
    assert p.to_bytes().hex() == PARENT["programs"][name]


def test_aggregate_programs_without_the_nodes_keep_the_bytes_of_the_parent():
    low = lower_aggregate(SCHEMA, KINDS, [Col("ts") >= Lit("1995-01-01"), Col("f") > Lit(1.0)], Col("a"),
                          [F.sum(Col("f") * Col("b")), F.min(Col("b")), F.sum(F.when(Col("ts") < Col("t2"), 1).otherwise(0)),
                           F.sum(Lit(1))], DICTS)
    low_ts = lower_aggregate(SCHEMA, KINDS, [Col("ts") >= Lit("1995-01-01")], Col("ts"), [F.sum(Col("f")), F.sum(Lit(1))], DICTS)
    for got, want in ((low, PARENT["aggregate"]), (low_ts, PARENT["aggregate_ts_key"])):
        assert got.program.to_bytes().hex() == want["program"]
        assert (got.key_slot, got.acc_ops, got.acc_is_int, got.agg_to_acc) == (
            want["key_slot"], want["acc_ops"], want["acc_is_int"], want["agg_to_acc"])


# ---- the stage lowering ------------------------------------------------------------------------------------------------
def test_int_bits_bounds_a_part_of_a_timestamp():
    from minispark_amd.stage import _int_bits

    want = {"year": 19, "quarter": 3, "month": 4, "day": 5, "hour": 5, "minute": 6, "second": 6, "dayofweek": 3, "dayofyear": 9}
    largest = {"year": 292_278, "quarter": 4, "month": 12, "day": 31, "hour": 23, "minute": 59, "second": 59, "dayofweek": 7, "dayofyear": 366}
    for name, fn in PART_FUNCTIONS.items():
        assert _int_bits(fn(Col("ts")), SCHEMA) == want[name] and largest[name] <= 1 << want[name]
        assert _int_bits(fn(F.date_trunc("week", Col("ts"))).alias("x"), SCHEMA) == want[name]
        assert _int_bits(fn(Col("a")), SCHEMA) is None and _int_bits(fn(Col("s")), SCHEMA) is None
        assert _int_bits(fn(Lit("1995-01-01")), SCHEMA) is None and _int_bits(fn(Col("nope")), SCHEMA) is None
    assert max(abs(model.part(0, I64_MIN)), model.part(0, I64_MAX)) <= 292_278 + 2000 < 1 << 19
    assert _int_bits(F.year(Col("ts")) * 12 + F.month(Col("ts")), SCHEMA) == 24
    assert _int_bits(F.date_trunc("day", Col("ts")), SCHEMA) is None  # a TIMESTAMP is no INTEGER key


def test_substitute_and_walk_names_rebuild_both_nodes():
    from minispark_amd.stage import _substitute, _walk_names

    defs = {"x": Col("ts"), "y": F.date_trunc("month", Col("t2")), "n": Col("a") + 1}
    got = _substitute(F.year(Col("x")) * 100 + F.month(Col("y")) + Col("n"), defs)
    assert str(got) == "(((YEAR(ts)) * (100)) + (MONTH(DATE_TRUNC('month', t2)))) + ((a) + (1))"
    node = _substitute(F.date_trunc("week", Col("x")).alias("w"), defs)
    assert type(node) is DateTruncColumn and node.unit == "week" and node.original_col is defs["x"]
    assert type(_substitute(F.dayofweek(Col("x")), defs)) is DatePartColumn
    assert _substitute(F.year(Col("ts")), None).part == "year"
    assert _walk_names(got) == ["ts", "t2", "a"]


def write_table(path: Path) -> None:
    from minispark_amd.io import BlockFile

    schema = [("d", ColumnType.TIMESTAMP), ("x", ColumnType.FLOAT), ("k", ColumnType.INTEGER)]
    base = model.to_cell(datetime(1995, 6, 1))
    blocks = [[np.array([base + i * 40 * US_PER_DAY for i in range(lo, lo + n)], dtype=np.int64),
               np.arange(lo, lo + n, dtype=np.float32), np.arange(lo, lo + n, dtype=np.int32) % 3] for lo, n in ((0, 5), (5, 7))]
    BlockFile(path).write_raw_blocks(schema, blocks)


def test_a_year_key_is_a_computed_key_of_the_scan_stage(tmp_path):
    from minispark_amd.stage import COMPUTED_KEY, StageUnsupported, lower_stage_plan

    path = tmp_path / "t.bin"
    write_table(path)
    frame = (DataFrame(object()).table(str(path)).select(F.year(Col("d")).alias("y"), Col("x"), Col("k")).filter(Col("k") != 1)
             .group_by(Col("y")).agg(F.sum(Col("x")).alias("s"), F.count()))
    blob, table, out_schema = lower_stage_plan(frame.task)
    assert blob.key_computed == 1 and Path(table) == path and [n for n, _ in out_schema] == ["y", "s", "count"]
    assert out_schema[0][1] == ColumnType.INTEGER
    key_words = [blob.key_prog.ins[i] for i in range(blob.key_prog.n_ins)]
    assert [(w & 0xff, (w >> 16) & 0xffff) for w in key_words] == [(hs.OP_LD, 0), (hs.OP_DATEPART, 0), (hs.OP_OUT, 0)]
    assert blob.n_kcols == 1 and blob.kcol_ids[0] == 0
    assert COMPUTED_KEY not in [n for n, _ in out_schema]
    # the SQL alias text lowers to the same stage
    sql = parse_sql(f"SELECT YEAR(d) AS y, SUM(x) AS s FROM '{path}' GROUP BY y;", object())
    blob2, _, _ = lower_stage_plan(sql.task)
    assert blob2.key_computed == 1 and bytes(blob2.key_prog) == bytes(blob.key_prog)
    # a part inside an aggregate's argument and the WHERE: ordinary value instructions of the scan's program
    inner = (DataFrame(object()).table(str(path)).filter(F.month(Col("d")) > 6).group_by(Col("k"))
             .agg(F.sum(F.when(F.year(Col("d")) == 1996, Col("x")).otherwise(0.0)).alias("s")))
    blob3, _, _ = lower_stage_plan(inner.task)
    ops = [blob3.prog.ins[i] & 0xff for i in range(blob3.prog.n_ins)]
    assert blob3.key_computed == 0 and ops.count(hs.OP_DATEPART) == 2
    # a TIMESTAMP-valued computed key is not materialised by the stage: refused as any non-INTEGER computed key is
    trunc = (DataFrame(object()).table(str(path)).select(F.date_trunc("month", Col("d")).alias("m"), Col("x"))
             .group_by(Col("m")).agg(F.sum(Col("x")).alias("s")))
    with pytest.raises(StageUnsupported, match="computed GROUP BY key"):
        lower_stage_plan(trunc.task)


# ---- the model inside the oracle ---------------------------------------------------------------------------------------
MODEL_SCHEMA = [("d", ColumnType.TIMESTAMP), ("a", ColumnType.INTEGER)]
MODEL_ROWS = [(datetime(2024, 2, 29, 23, 59, 59), 1), (datetime(1969, 12, 31, 23, 59, 59), 2), (datetime(2023, 1, 1), 3),
              (datetime(1900, 3, 1, 12, 30), 4)]


@pytest.mark.parametrize("expr,want", [
    (lambda: F.year(Col("d")), [2024, 1969, 2023, 1900]),
    (lambda: F.dayofyear(Col("d")) * 10 + F.dayofweek(Col("d")), [604, 3653, 17, 604]),
    (lambda: F.date_trunc("month", Col("d")), [datetime(2024, 2, 1), datetime(1969, 12, 1), datetime(2023, 1, 1), datetime(1900, 3, 1)]),
    (lambda: F.date_trunc("week", Col("d")), [datetime(2024, 2, 26), datetime(1969, 12, 29), datetime(2022, 12, 26), datetime(1900, 2, 26)]),
    (lambda: F.quarter(F.date_trunc("year", Col("d"))) + Col("a"), [2, 3, 4, 5]),
    (lambda: F.when(F.month(Col("d")) == 2, F.day(Col("d"))).otherwise(0), [29, 0, 0, 0]),
    (lambda: F.date_trunc("hour", Col("d")) > Lit(datetime(1969, 12, 31, 23)), [True, False, True, False]),
])
def test_the_model_on_rows_computed_by_hand(monkeypatch, expr, want):
    model.install(monkeypatch)
    fn = py_engine.compile_expr(expr(), MODEL_SCHEMA)
    got = [fn(row) for row in MODEL_ROWS]
    assert got == want and [type(v) for v in got] == [type(v) for v in want]


def test_the_model_leaves_every_other_node_to_the_oracle(monkeypatch):
    plain = (Col("a") + 1) * Col("a")
    before = [py_engine.compile_expr(plain, MODEL_SCHEMA)(row) for row in MODEL_ROWS]
    with pytest.raises(NotImplementedError):
        py_engine.compile_expr(F.year(Col("d")), MODEL_SCHEMA)
    model.install(monkeypatch)
    assert [py_engine.compile_expr(plain, MODEL_SCHEMA)(row) for row in MODEL_ROWS] == before
    with pytest.raises(TypeError, match="TIMESTAMP"):
        py_engine.compile_expr(F.year(Col("a")), MODEL_SCHEMA)(MODEL_ROWS[0])


# ---- the run-time compiler: translate + compile for gfx950, no GPU needed ------------------------------------------------
def _hs_cols(program, kinds):
    cols = (hs.hs_col * max(len(program.columns), 1))()
    for slot, idx in enumerate(program.columns):
        coded = idx in program.code_columns
        cols[slot].kind = hs.U8 if coded else kinds[idx]
        cols[slot].fixed_len = 1 if (kinds[idx] == hs.STR and not coded) else -1
    return cols


ALL_SELECTORS = [*range(9), *range(16, 24)]


def check_datepart_programs_compile():
    """hs_jit_compile_check / _scalar / _eval on programs holding every selector: COMPILED, not declined to the interpreter;
    each call is one hs_datepart_c<selector> with the selector as a template argument, and a part of a literal is hoisted
    out of the row loop."""
    lib = hs.load_library()
    ts = Col("ts")
    aggs = [F.sum(F.when(F.year(ts) == 1996, Col("f")).otherwise(0)), F.max(F.quarter(ts) * 10 + F.dayofweek(ts)),
            F.sum(F.hour(ts) * 3600 + F.minute(ts) * 60 + F.second(ts)), F.min(F.dayofyear(F.date_trunc("week", ts))),
            F.sum(F.year(Lit(datetime(2024, 2, 29)))),
            F.sum(F.when(F.date_trunc("quarter", ts) >= "1995-01-01", 1).otherwise(0)),
            F.max(F.day(F.date_trunc("month", F.date_trunc("year", Col("t2"))))),
            F.sum(F.when((F.date_trunc("day", ts) == F.date_trunc("hour", Col("t2"))) |
                         (F.date_trunc("minute", ts) == F.date_trunc("second", Col("t2"))), 1).otherwise(0))]
    where = [(F.month(ts) == 2) & (F.day(ts) == 29)]
    for keyed in (True, False):
        low = lower_aggregate(SCHEMA, KINDS, where, Col("a") if keyed else None, aggs, DICTS)
        selectors = [i[2] for i in ins(low.program) if i[0] == hs.OP_DATEPART]
        assert sorted(set(selectors)) == ALL_SELECTORS
        cols = _hs_cols(low.program, KINDS)
        prog, spec = low.program.to_struct(), low.spec()
        src, size = C.create_string_buffer(1 << 16), C.c_int64(0)
        if keyed:
            rc = lib.hs_jit_compile_check(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                          C.byref(size), src, len(src))
        else:
            rc = lib.hs_jit_compile_check_scalar(cols, len(low.program.columns), C.byref(prog), C.byref(spec), b"gfx950",
                                                 C.byref(size), src, len(src))
        assert rc == 0, (keyed, lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
        text = src.value.decode()
        assert text.count("hs_datepart_c<") == len(selectors) and size.value > 4096
        for sel in ALL_SELECTORS:
            assert f"hs_datepart_c<{sel}u>(" in text
        head, _, body = text.partition("for (int j = 0; j < HS_V; ++j)")
        hoisted = [line for line in head.splitlines() if "hs_datepart_c<" in line]
        assert len(hoisted) == 1 and hoisted[0].strip().startswith("const unsigned long long k") and "hs_datepart_c<0u>(k" in hoisted[0]
        assert body.count("hs_datepart_c<") == len(selectors) - 1
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    exprs = [fn(ts) for fn in PART_FUNCTIONS.values()] + [F.date_trunc(u, Col("t2")) for u in hs.DATE_TRUNC_UNITS[:6]]
    exprs.append(F.date_trunc("minute", ts) == F.date_trunc("second", Col("t2")))
    tags = [b.emit_out(o, e) for o, e in enumerate(exprs)]
    assert tags == ["I"] * 9 + ["T"] * 6 + ["B"] and len(exprs) == hs.HS_MAX_OUTS
    program = b.finish()
    cols = _hs_cols(program, KINDS)
    pstruct, size, src = program.to_struct(), C.c_int64(0), C.create_string_buffer(1 << 16)
    out_kinds = (C.c_int32 * 16)(*[hs.I64] * 15, hs.U8)
    rc = lib.hs_jit_compile_check_eval(cols, len(program.columns), C.byref(pstruct), out_kinds, 16, b"gfx950", C.byref(size), src, len(src))
    assert rc == 0, (lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
    assert src.value.decode().count("hs_datepart_c<") == 17 and size.value > 1000


def test_programs_with_every_selector_translate_and_compile_for_gfx950_without_a_gpu():
    check_datepart_programs_compile()


def test_the_generators_decline_a_selector_out_of_range_and_a_stack_underflow():
    lib = hs.load_library()

    def word(op, sp, a=0):
        return op | (sp << 8) | (a << 16)

    cols = (hs.hs_col * 1)()
    cols[0].kind, cols[0].fixed_len = hs.I64, -1
    out_kinds = (C.c_int32 * 1)(hs.I64)
    for words, why in (([word(hs.OP_LD, 0, 0), word(hs.OP_DATEPART, 1, 9), word(hs.OP_OUT, 1, 0)], "selector"),
                       ([word(hs.OP_LD, 0, 0), word(hs.OP_DATEPART, 1, 24), word(hs.OP_OUT, 1, 0)], "selector"),
                       ([word(hs.OP_DATEPART, 0, 0)], "underflow")):
        p = hs.hs_program()
        p.n_ins = len(words)
        for i, w in enumerate(words):
            p.ins[i] = w
        size, src = C.c_int64(0), C.create_string_buffer(1 << 14)
        rc = lib.hs_jit_compile_check_eval(cols, 1, C.byref(p), out_kinds, 1, b"gfx950", C.byref(size), src, len(src))
        assert rc != 0 and why in lib.hs_last_error().decode(), (words, lib.hs_last_error())


def test_the_host_side_program_checks_take_datepart_as_a_value_instruction():
    """hs_agg_rows_classify walks `[filter ... FILTER]* KEY [argument ... AGG]*`: a part as an argument is an expression cell
    (kind HS_I64, no bare column, no literal), parts in the WHERE are one filter."""
    lib = hs.load_library()
    ts = Col("ts")
    low = lower_aggregate(SCHEMA, KINDS, [(F.month(ts) == 2) & (F.day(ts) == 29)], Col("a"),
                          [F.sum(F.year(ts)), F.sum(F.when(F.year(ts) == 1996, Col("f")).otherwise(0)), F.sum(Col("f")), F.sum(Lit(1))])
    cols = _hs_cols(low.program, KINDS)
    prog, spec = low.program.to_struct(), low.spec()
    kinds, slots, cells, n_filters = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_uint64 * 4)(), C.c_int32(-1)
    rc = lib.hs_agg_rows_classify(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), kinds, slots, cells,
                                  C.byref(n_filters))
    assert rc == 0, lib.hs_last_error()
    assert n_filters.value == 1
    assert list(kinds) == [hs.I64, hs.F64, hs.F32, -1] and list(slots)[:2] == [-1, -1] and cells[3] == 1
