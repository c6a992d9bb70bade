"""Plain Python statement of ONE partial-aggregate scan - rows -> per-unit partial rows as the reference's shuffle file
would hold them - and the edge table every tier is held to (tests/test_gpu_agg_scan_edges.py on the device, pinned
against the oracle without one by tests/test_agg_scan_model_cpu.py).

The fold is tests/agg_tail_models.py's ``fold`` from the INT identities (oracle/py_engine.py:135-150: ``min(MAX_INT, x)``
keeps the int unless x is strictly smaller), aggregate arguments are evaluated by ``oracle.py_engine.compile_expr`` and a
cell is stored by ``agg_tail_models.store``.  A cell the reference has no bytes for - a FLOAT MIN / MAX that still holds the
int identity, a store that raises, a quotient by zero - is ``None`` next to its flag.

The data keeps four conditions, asserted by ``build_table`` itself:

* exact sums: the finite FLOAT addends of a group are multiples of one power of two and their magnitudes add up to less
  than 2^53 of those quanta, so every association gives the same f64 sum (the LDS tiers add in hardware order);
* -0.0 appears nowhere (DESIGN.md 2 leaves the sign of a MIN / MAX over both zeros open);
* a NaN result is compared as "is NaN" only (``cell_token``);
* nothing is skipped beyond the ``None`` cells of a raising scenario's affected aggregates.
"""

from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache

import numpy as np

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType as T
from minispark_amd.sql import Col, Functions as F
from oracle.py_engine import compile_expr
from tests.agg_tail_models import MAX, MIN, SUM, fold, identity, store

SCHEMA = [("k", T.INTEGER), ("keep", T.INTEGER), ("f", T.FLOAT), ("d", T.FLOAT), ("i", T.INTEGER)]
UNIT_SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 70_001]
BOUNDS = [0]
for _size in UNIT_SIZES:
    BOUNDS.append(BOUNDS[-1] + _size)
N_ROWS = BOUNDS[-1]
LONG_UNIT = len(UNIT_SIZES) - 1

INT32_MAX, INT32_MIN = 2**31 - 1, -(2**31)
FLT_MAX = float(np.finfo(np.float32).max)  # (2^24 - 1) * 2^104
_OPS = {"sum": SUM, "min": MIN, "max": MAX}


# ---- the two programs ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScanProgram:
    name: str
    aggs: tuple  # AggCol with an alias

    @property
    def filters(self) -> list:
        return [Col("keep") == 1]

    @property
    def names(self) -> list[str]:
        return [a.name for a in self.aggs]

    @property
    def ops(self) -> list[int]:
        return [_OPS[a.type] for a in self.aggs]

    @property
    def kinds(self) -> list[int]:
        return [hs.I32 if a.infer_type(SCHEMA) == T.INTEGER else hs.F32 for a in self.aggs]

    @property
    def out_schema(self) -> list:
        return [("k", T.INTEGER)] + [(a.name, a.infer_type(SCHEMA)) for a in self.aggs]


def programs() -> dict[str, ScanProgram]:
    """Both programs run under WHERE keep == 1.  "six": Q1's accumulator count; "quot": an argument that can divide by zero."""
    f, d, i = Col("f"), Col("d"), Col("i")
    return {
        "six": ScanProgram("six", (F.sum(f).alias("sf"), F.min(f).alias("nf"), F.max(f).alias("xf"),
                                   F.sum(i).alias("si"), F.min(i).alias("ni"), F.max(i).alias("xi"))),
        "quot": ScanProgram("quot", (F.sum(f / d).alias("sq"), F.min(f).alias("nf"))),
    }


# ---- the scenarios ------------------------------------------------------------------------------------------------
def _nan(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


NAN_A, NAN_B = 0x7FC00001, 0xFFA5A5A5  # a quiet NaN with a payload, a negative signalling one


@dataclass(frozen=True)
class Scenario:
    """One group.  rows: (f, d, i, keep).  A raising scenario names, per program it raises in, the flag, the oracle's
    exception and the aggregates whose cells the reference has no bytes for."""
    name: str
    rows: tuple
    raising: tuple = ()  # (program, flag, exception type, (aggregate names))

    def raises_in(self, program: str):
        """-> (flag, exception type, aggregate names) or None"""
        return next((entry[1:] for entry in self.raising if entry[0] == program), None)


def _rows(fs=None, ints=None, d=1.0):
    n = len(fs if fs is not None else ints)
    fs = fs if fs is not None else [0.5 * (j + 1) for j in range(n)]
    ints = ints if ints is not None else [3 * j - 4 for j in range(n)]
    return tuple((f, d, i, 1) for f, i in zip(fs, ints))


QUIET = [
    Scenario("nan_among_finite", _rows([1.5, _nan(NAN_A), -2.25, _nan(NAN_B), 4.0])),
    Scenario("inf_among_finite", _rows([1.0, math.inf, -3.5])),
    Scenario("both_infinities", _rows([math.inf, 2.0, -math.inf])),
    Scenario("flt_max_both_signs", _rows([FLT_MAX, -FLT_MAX, 3 * 2.0**104])),
    Scenario("tiny_positive", _rows([2.0**-149, 2.0**-126, 3 * 2.0**-149])),
    Scenario("tiny_negative", _rows([-(2.0**-149), -(2.0**-126), -3 * 2.0**-149])),
    Scenario("denormal_sum", _rows([5 * 2.0**-149, 7 * 2.0**-149, -2 * 2.0**-149])),
    Scenario("sum_rounds_down_to_flt_max", _rows([FLT_MAX, 2.0**103, -(2.0**102)])),  # FLT_MAX + 2^102: below half an ulp
    Scenario("min_just_below_2_31", _rows([2147483520.0, 3e9])),
    Scenario("max_just_above_minus_2_31", _rows([-2147483520.0, -3e9])),
    Scenario("int_sum_reaches_int32_max", _rows(ints=[2**30, 0, 2**30 - 1])),
    Scenario("int_sum_reaches_int32_min", _rows(ints=[-(2**30), -(2**30)])),
    Scenario("int_extremes", _rows(ints=[INT32_MAX, INT32_MIN, 0])),
    Scenario("dead_rows_hold_the_edges", (
        (1.0, 1.0, 5, 1), (_nan(NAN_A), 0.0, INT32_MAX, 0), (math.inf, 0.0, INT32_MAX, 0), (2.0, 2.0, -7, 1),
        (-math.inf, 0.0, INT32_MIN, 0), (float(np.float32(3e38)), 0.0, INT32_MAX, 0), (float(np.float32(3e38)), 0.0, 1, 0))),
]
_TA, _FO, _IO, _DZ = hs.FLAG_TYPE_ASSERT, hs.FLAG_FLT_OVERFLOW, hs.FLAG_INT_OVERFLOW, hs.FLAG_DIV_ZERO
RAISING = [
    Scenario("only_nan", _rows([_nan(NAN_A), _nan(NAN_B)]),
             (("six", _TA, AssertionError, ("nf", "xf")), ("quot", _TA, AssertionError, ("nf",)))),
    Scenario("only_plus_inf", _rows([math.inf, math.inf]),
             (("six", _TA, AssertionError, ("nf",)), ("quot", _TA, AssertionError, ("nf",)))),
    Scenario("only_2_31_and_above", _rows([2147483648.0, 3e9]),
             (("six", _TA, AssertionError, ("nf",)), ("quot", _TA, AssertionError, ("nf",)))),
    Scenario("only_minus_2_31", _rows([-2147483648.0, -2147483648.0]), (("six", _TA, AssertionError, ("xf",)),)),
    Scenario("sum_rounds_up_to_2_128", _rows([FLT_MAX, 2.0**104, -(2.0**103)]),  # FLT_MAX + 2^103: half-way, to even = 2^128
             (("six", _FO, OverflowError, ("sf",)), ("quot", _FO, OverflowError, ("sq",)))),
    Scenario("int_sum_int32_max_plus_1", _rows(ints=[2**30, 2**30]), (("six", _IO, OverflowError, ("si",)),)),
    # the row that divides by zero is not the group's MIN(f): whether such a row still reaches the other aggregates
    # is nothing the reference can tell (its job is over)
    Scenario("live_divisor_zero", ((1.0, 1.0, 1, 1), (2.0, 0.0, 2, 1), (3.0, 1.0, 3, 1)),
             (("quot", _DZ, ZeroDivisionError, ("sq",)),)),
]
SCENARIOS = {s.name: s for s in QUIET + RAISING}
FILLER_KEYS = (0, 1)
SCENARIO_KEY = {name: 100 + j for j, name in enumerate(SCENARIOS)}


# ---- the table ----------------------------------------------------------------------------------------------------
def _long_unit_slots() -> list[int]:
    """Rows of the long unit that take scenario rows, alternating between its two 65 536-row halves: workgroup (1024) and
    chunk (65 536) boundaries from both sides, quad and wave boundaries, the first and the last row."""
    low = [1023, 1024, 1025, 0, 3, 4, 63, 64, 2047, 2048, 255, 256, 4095, 4096, 7, 8, 1, 2, 32767, 32768,
           3071, 3072, 5119, 5120, 16383, 16384, 511, 512, 6143, 6144, 65531, 65532]
    high = [65536, 65535, 65537, 70000, 66559, 66560, 69999, 67583, 67584, 65539, 65540, 68607, 68608, 69631, 69632,
            65599, 65600, 69996, 69997, 66047, 66048, 65791, 65792, 69995, 67071, 67072, 68095, 68096, 69119, 69120,
            65543, 65544]
    out = [row for pair in zip(low, high) for row in pair]
    assert len(set(out)) == len(out) and max(out) < UNIT_SIZES[LONG_UNIT]
    return out


def _small_unit_slots(size: int) -> list[int]:
    want = [0, size - 1, 3, 4, 1, size - 2, 7, 8, 63, 64, 2, 5]
    return list(dict.fromkeys(r for r in want if 0 <= r < size))


@dataclass
class EdgeTable:
    columns: dict                      # name -> numpy array in SCHEMA order and kind
    scenarios: tuple
    placed: dict = field(default_factory=dict)  # scenario -> [units holding a complete copy of its rows]

    def python_columns(self) -> list[list]:
        return [self.columns[name].tolist() for name, _ in SCHEMA]

    def blocks(self) -> list[list]:
        """The raw columns cut at the unit boundaries (BlockFile.write_raw_blocks)."""
        return [[self.columns[name][lo:hi] for name, _ in SCHEMA] for lo, hi in zip(BOUNDS, BOUNDS[1:])]


def build_table(scenarios: tuple, filler_keys: tuple = FILLER_KEYS, filler_live: bool = True, copies: bool = True) -> EdgeTable:
    """The edge table holding `scenarios` (names): every scenario's rows sit COMPLETE in the long unit - spread over both of
    its chunks - and, with `copies`, once more in a small unit where one has room, at first / last rows and quad boundaries
    (a whole query merges the units, so it takes one copy: two would change the scenario's sum).  Every other
    row is ordinary: k/8 values under `filler_keys`, every fifth of them dead (keep = 0) with NaN / inf / 3e38, d = 0.0 and an
    int extreme.  filler_live=False kills all of them (the keyless scan: a scenario is then the whole table)."""
    r = np.arange(N_ROWS)
    keys = np.asarray(filler_keys if filler_keys else (0,), dtype=np.int32)
    k = keys[r % len(keys)]
    keep = np.where(r % 5 == 2, 0, 1).astype(np.int32) if filler_live else np.zeros(N_ROWS, dtype=np.int32)
    nasty = np.array([_nan(NAN_B), math.inf, -math.inf, 3e38], dtype=np.float32)
    dead = r % 5 == 2
    f = np.where(dead, nasty[r % 4], (((r * 7) % 33) - 16) / 8.0).astype(np.float32)
    d = np.where(dead, 0.0, np.array([1.0, 2.0, 0.5, 4.0])[r % 4]).astype(np.float32)
    i = np.where(dead, INT32_MAX, (r * 13) % 2001 - 1000).astype(np.int32)
    table = EdgeTable({"k": k.copy(), "keep": keep, "f": f, "d": d, "i": i}, tuple(scenarios))

    def put(row: int, key: int, cells: tuple) -> None:
        table.columns["k"][row] = key
        table.columns["f"][row], table.columns["d"][row], table.columns["i"][row], table.columns["keep"][row] = cells

    long_slots = iter(_long_unit_slots())
    free = {u: _small_unit_slots(size) for u, size in enumerate(UNIT_SIZES[:-1])}
    for j, name in enumerate(scenarios):
        sc, key = SCENARIOS[name], SCENARIO_KEY[name]
        table.placed[name] = [LONG_UNIT]
        for cells in sc.rows:
            put(BOUNDS[LONG_UNIT] + next(long_slots), key, cells)
        for step in range(len(free) if copies else 0):
            u = (j + step) % len(free)
            if len(free[u]) >= len(sc.rows):
                for cells in sc.rows:
                    put(BOUNDS[u] + free[u].pop(0), key, cells)
                table.placed[name].append(u)
                break
    for program in programs().values():
        check_conditions(table, program)
    return table


def _quantum(x: float) -> Fraction:
    """The largest power of two that x is an integer multiple of."""
    fr = Fraction(x)
    return Fraction(fr.numerator & -fr.numerator, fr.denominator)  # the denominator of a float is a power of two


def check_conditions(table: EdgeTable, program: ScanProgram) -> None:
    """Exact sums and zero signs (module docstring), per group over the whole table, on the aggregate arguments of the
    rows that pass the filter."""
    live = [compile_expr(c, SCHEMA) for c in program.filters]
    args = [(a, compile_expr(agg, SCHEMA)) for a, agg in enumerate(program.aggs) if program.kinds[a] == hs.F32]
    seen: dict = {}  # (group, aggregate, value, its sign) -> rows
    for row in zip(*table.python_columns()):
        if not all(fn(row) for fn in live):
            continue
        for a, fn in args:
            try:
                x = fn(row)
            except ZeroDivisionError:
                continue
            cell = (row[0], a, x, math.copysign(1.0, x))  # (0.0 == -0.0: the sign keeps them apart)
            seen[cell] = seen.get(cell, 0) + 1
    addends: dict = {}
    for (key, a, x, sign), n in seen.items():
        assert not (x == 0.0 and sign < 0), f"-0.0 in group {key}"
        if program.ops[a] == SUM and math.isfinite(x) and x != 0.0:
            count = addends.setdefault((key, a), {})
            count[abs(x)] = count.get(abs(x), 0) + n
    for (key, a), count in addends.items():
        q = min(_quantum(x) for x in count)
        total = sum(Fraction(x) * n for x, n in count.items()) / q
        assert total < 2**53, f"group {key}, {program.names[a]}: {float(total):.3g} quanta of {float(q):.3g}: the sum depends on its order"


# ---- the model ----------------------------------------------------------------------------------------------------
def scan_model(columns: list[list], bounds: list[int], program: ScanProgram, keyless: bool = False):
    """rows -> ([{key: [stored bytes or None per aggregate]} per unit], OR of the flags).  A unit's rows that pass the
    filter are folded per group in row order; keyless: under the one key 0."""
    live = [compile_expr(c, SCHEMA) for c in program.filters]
    args = [compile_expr(a, SCHEMA) for a in program.aggs]
    ops, kinds = program.ops, program.kinds
    rows = list(zip(*columns))
    units, flags = [], 0
    for lo, hi in zip(bounds, bounds[1:]):
        accs: dict = {}
        no_value: dict = {}
        for row in rows[lo:hi]:
            if not all(fn(row) for fn in live):
                continue
            key = 0 if keyless else row[0]
            acc = accs.get(key)
            if acc is None:
                acc = accs[key] = [identity(op, True) for op in ops]  # the reference starts every aggregate from an int
            for a, fn in enumerate(args):
                try:
                    acc[a] = fold(ops[a], acc[a], fn(row))
                except ZeroDivisionError:
                    flags |= hs.FLAG_DIV_ZERO
                    no_value.setdefault(key, set()).add(a)
        out = {}
        for key, acc in accs.items():
            cells = []
            for a, value in enumerate(acc):
                if a in no_value.get(key, ()):
                    cells.append(None)
                elif kinds[a] == hs.F32 and type(value) is int:  # io.py:93: a FLOAT column holds an int
                    flags |= hs.FLAG_TYPE_ASSERT
                    cells.append(None)
                else:
                    data, raised = store(value, kinds[a])
                    flags |= raised
                    cells.append(data)
            out[key] = cells
        units.append(out)
    return units, flags


def cell_token(data, kind: int):
    """What two stored cells are compared by: the 32 bits, "nan" for every f32 NaN, None for a cell without bytes."""
    if data is None:
        return None
    (bits,) = struct.unpack("<I", bytes(data))
    if kind == hs.F32 and (bits & 0x7F800000) == 0x7F800000 and (bits & 0x007FFFFF):
        return "nan"
    return bits


def unit_tokens(units: list[dict], kinds: list[int]) -> list[dict]:
    return [{key: tuple(cell_token(c, kind) for c, kind in zip(cells, kinds)) for key, cells in unit.items()} for unit in units]


@lru_cache(maxsize=None)
def expected(scenarios: tuple, filler_keys: tuple, filler_live: bool, program: str, keyless: bool = False,
             copies: bool = True):
    """(table, per-unit {key: cell tokens}, flags) of one launch - computed once, shared by every tier, never changed."""
    table = build_table(scenarios, filler_keys, filler_live, copies)
    prog = programs()[program]
    units, flags = scan_model(table.python_columns(), BOUNDS, prog, keyless)
    return table, unit_tokens(units, prog.kinds), flags


def undefined_cells(tokens: list[dict]) -> set:
    return {(u, key, a) for u, unit in enumerate(tokens) for key, cells in unit.items() for a, c in enumerate(cells) if c is None}


def expected_undefined(table: EdgeTable, program: ScanProgram, keyless: bool = False) -> set:
    """The cells a launch may leave uncompared: per scenario that raises in this program, its affected aggregates in every
    unit that holds a copy of the group."""
    out = set()
    for name in table.scenarios:
        entry = SCENARIOS[name].raises_in(program.name)
        for u in table.placed[name] if entry else ():
            out |= {(u, 0 if keyless else SCENARIO_KEY[name], program.names.index(agg)) for agg in entry[2]}
    return out


def expected_flags(table: EdgeTable, program: ScanProgram) -> int:
    flags = 0
    for name in table.scenarios:
        entry = SCENARIOS[name].raises_in(program.name)
        flags |= entry[0] if entry else 0
    return flags


# ---- the launches -------------------------------------------------------------------------------------------------
def _launches() -> dict[str, list[tuple]]:
    """(scenarios, filler keys, filler live) per launch.  "wide": every quiet scenario in one launch, then every raising one
    alone next to the ordinary groups.  "narrow": the same four groups at a time (what the private tables hold at six
    accumulators).  "keyless": every scenario is its own one-group table, and the ordinary rows are one more."""
    quiet, raising = [s.name for s in QUIET], [s.name for s in RAISING]
    return {
        "wide": [(tuple(quiet), FILLER_KEYS, True)] + [((name,), FILLER_KEYS, True) for name in raising],
        "narrow": [(tuple(quiet[j: j + 3]), FILLER_KEYS[:1], True) for j in range(0, len(quiet), 3)]
                  + [((name,), FILLER_KEYS[:1], True) for name in raising],
        "keyless": [((), FILLER_KEYS, True)] + [((name,), (), False) for name in quiet + raising],
    }


LAUNCHES = _launches()
