"""CPU model of the date functions for the tests: a pure-integer restatement of DESIGN.md 4.4d on the microsecond cell, and
the oracle's ``compile_expr`` with two more node classes.

The calendar.  A TIMESTAMP cell is a signed 64-bit count of microseconds since 1970-01-01T00:00:00; parts are those of the
proleptic Gregorian calendar without a time zone; division is floor division (Python's ``//`` and ``%``); the functions are
total over i64.  ``part(sel, cell)`` restates HS_OP_DATEPART selector by selector with Python integers - the
``civil_from_days`` / ``days_from_civil`` construction over 400-year eras of 146 097 days - and truncations wrap to 64 bits
as the device's arithmetic does (only a unit that starts before the first representable microsecond wraps).  The tests
check this model against numpy's datetime64 and against ``datetime``, so the GPU is compared with a calendar two other
implementations agree on.

The oracle (oracle/py_engine.py) dispatches on class names and knows neither ``DatePartColumn`` nor ``DateTruncColumn``.
``compile_expr`` below handles the two and hands every other node to the oracle's own function; installed with

    monkeypatch.setattr(oracle.py_engine, "compile_expr", date_part_model.compile_expr)

nested and aggregated calls go through the model too, and the oracle's quantisation points, per-block partial sums and
merge order apply unchanged.  Rows hold ``datetime`` values (naive, read under TZ=UTC): they are turned into the cell and
back with integer arithmetic, never through a float.  CASE WHEN is handled as tests/case_when_model.py does, so a part may
stand inside a CASE.
"""

from __future__ import annotations

from datetime import datetime, timedelta
from typing import Any, Callable

import numpy as np

import oracle.py_engine as py_engine
from tests import case_when_model

US_PER_DAY = 86_400_000_000
PARTS = ("year", "quarter", "month", "day", "hour", "minute", "second", "dayofweek", "dayofyear")  # selectors 0 .. 8
UNITS = ("year", "quarter", "month", "week", "day", "hour", "minute", "second")                   # selectors 16 .. 23
TRUNC_BASE = 16
_EPOCH = datetime(1970, 1, 1)
_US = timedelta(microseconds=1)


def _where(cond: Any, a: Any, b: Any) -> Any:
    return np.where(cond, a, b) if isinstance(cond, np.ndarray) else (a if cond else b)


def civil_from_days(days: Any) -> tuple[Any, Any, Any]:
    """day number (1970-01-01 = 0) -> (year, month, day)"""
    z = days + 719_468  # days since 0000-03-01
    era, doe = divmod(z, 146_097)
    yoe = (doe - doe // 1460 + doe // 36_524 - doe // 146_096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)  # March-based
    mp = (5 * doy + 2) // 153
    day = doy - (153 * mp + 2) // 5 + 1
    month = _where(mp < 10, mp + 3, mp - 9)
    return yoe + era * 400 + _where(month <= 2, 1, 0), month, day


def days_from_civil(year: Any, month: Any, day: Any) -> Any:
    year = year - _where(month <= 2, 1, 0)
    era, yoe = divmod(year, 400)
    doy = (153 * _where(month > 2, month - 3, month + 9) + 2) // 5 + day - 1
    return era * 146_097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719_468


def wrap(value: Any) -> Any:
    """two's-complement i64 (an int64 array has wrapped already)"""
    if isinstance(value, np.ndarray):
        return value
    return (value + (1 << 63)) % (1 << 64) - (1 << 63)


def part(sel: int, cell: Any) -> Any:
    """HS_OP_DATEPART: selector 0 .. 8 a part, 16 .. 23 a truncation; ``cell`` and the result are signed 64-bit integers -
    a Python int, or a numpy int64 array (the same integer operations, element by element)."""
    days, us = divmod(cell, US_PER_DAY)
    second_of_day = us // 1_000_000
    year, month, day = civil_from_days(days)
    weekday = (days + 3) % 7 + 1  # ISO; 1970-01-01 is a Thursday
    if sel == 0:
        return year
    if sel == 1:
        return (month + 2) // 3
    if sel == 2:
        return month
    if sel == 3:
        return day
    if sel == 4:
        return second_of_day // 3600
    if sel == 5:
        return second_of_day // 60 % 60
    if sel == 6:
        return second_of_day % 60
    if sel == 7:
        return weekday
    if sel == 8:
        return days - days_from_civil(year, 1, 1) + 1
    if sel == 16:
        return wrap(days_from_civil(year, 1, 1) * US_PER_DAY)
    if sel == 17:
        return wrap(days_from_civil(year, (month - 1) // 3 * 3 + 1, 1) * US_PER_DAY)
    if sel == 18:
        return wrap(days_from_civil(year, month, 1) * US_PER_DAY)
    if sel == 19:
        return wrap((days - (weekday - 1)) * US_PER_DAY)
    if sel == 20:
        return wrap(days * US_PER_DAY)
    if sel == 21:
        return wrap(cell - us % 3_600_000_000)
    if sel == 22:
        return wrap(cell - us % 60_000_000)
    if sel == 23:
        return wrap(cell - us % 1_000_000)
    raise ValueError(f"selector {sel}")


def selector(node: Any) -> int:
    if type(node).__name__ == "DatePartColumn":
        return PARTS.index(node.part)
    return TRUNC_BASE + UNITS.index(node.unit)


def to_cell(value: datetime) -> int:
    return (value - _EPOCH) // _US


def from_cell(cell: int) -> datetime:
    return _EPOCH + cell * _US


_oracle_compile_expr = py_engine.compile_expr  # the oracle's own, bound before any test patches the module


def compile_expr(expr: Any, schema: list[tuple[str, Any]]) -> Callable[[tuple], Any]:
    kind = type(expr).__name__
    if kind == "CaseColumn":
        return case_when_model.compile_expr(expr, schema)  # its operands: py_engine.compile_expr = this function while installed
    if kind not in ("DatePartColumn", "DateTruncColumn"):
        return _oracle_compile_expr(expr, schema)
    inner = py_engine.compile_expr(expr.original_col, schema)  # looked up at call time: this function while installed
    sel = selector(expr)

    def run(row: tuple) -> Any:
        value = inner(row)
        if type(value) is not datetime:
            raise TypeError(f"{expr}: the argument of a date function is a TIMESTAMP value, not {type(value).__name__}")
        result = part(sel, to_cell(value))
        return result if sel < TRUNC_BASE else from_cell(result)

    return run


def install(monkeypatch: Any) -> None:
    """For the duration of the test: the oracle evaluates the date functions (and CASE WHEN) through the model."""
    monkeypatch.setattr(py_engine, "compile_expr", compile_expr)
