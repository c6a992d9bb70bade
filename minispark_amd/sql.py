"""Expression IR of the hot path: what WHERE predicates, projections and aggregate arguments are made of.

Host-side mirror of the reference's ``mini_spark.sql`` surface (reference: src/mini_spark/sql.py) so that
queries written against the reference (``Col("a") * Col("b")``, ``F.sum(...)``, ``.alias()``, ``.like()``,
``.between()``) build the same trees with the same *auto-generated column names* (they are visible in
result rows: ``quantity_add_lit_3``, ``sum_quantity``, ``count`` ... sql.py:260,369,409,464).

Nothing in here evaluates rows.  Trees are (1) type-checked with the reference's promotion rules
(``infer_type``; sql.py:277-303) and (2) lowered to device bytecode by :mod:`minispark_amd.lowering`,
which dispatches on class *names* and the attribute names kept here (``left_side``, ``right_side``,
``operator``, ``original_col``, ``pattern``, ``value``, ``type``) - so the reference's own objects lower
through the same code when the engine is plugged into the reference.
"""

from __future__ import annotations

import operator as _op
import re
from datetime import datetime
from typing import Any, Callable, Iterable, Iterator

from .constants import ColumnType, ColumnTypePython, Schema

BINOP_SYMBOLS: dict[Callable[..., Any], str] = {
    _op.add: "+",
    _op.sub: "-",
    _op.mul: "*",
    _op.truediv: "/",
    _op.floordiv: "//",
    _op.mod: "%",
    _op.eq: "==",
    _op.ne: "!=",
    _op.lt: "<",
    _op.le: "<=",
    _op.gt: ">",
    _op.ge: ">=",
    _op.and_: "and",
    _op.or_: "or",
}


def _wrap(value: Any) -> "Col":
    return value if isinstance(value, Col) else Lit(value)


class Col:
    """Reference to a column by name; also the base class of every expression node."""

    def __init__(self, name: str) -> None:
        self.name = name

    # -- expression builders ---------------------------------------------------------------------------
    def _bin(self, other: Any, fn: Callable[..., Any]) -> "Col":
        return BinaryOperatorColumn(self, _wrap(other), fn)

    def __add__(self, o: Any) -> "Col":
        return self._bin(o, _op.add)

    def __sub__(self, o: Any) -> "Col":
        return self._bin(o, _op.sub)

    def __mul__(self, o: Any) -> "Col":
        return self._bin(o, _op.mul)

    def __truediv__(self, o: Any) -> "Col":
        return self._bin(o, _op.truediv)

    def __floordiv__(self, o: Any) -> "Col":
        return self._bin(o, _op.floordiv)

    def __mod__(self, o: Any) -> "Col":
        return self._bin(o, _op.mod)

    def __lt__(self, o: Any) -> "Col":
        return self._bin(o, _op.lt)

    def __le__(self, o: Any) -> "Col":
        return self._bin(o, _op.le)

    def __gt__(self, o: Any) -> "Col":
        return self._bin(o, _op.gt)

    def __ge__(self, o: Any) -> "Col":
        return self._bin(o, _op.ge)

    def __eq__(self, o: Any) -> "Col":  # type: ignore[override]
        return self._bin(o, _op.eq)

    def __ne__(self, o: Any) -> "Col":  # type: ignore[override]
        return self._bin(o, _op.ne)

    def __and__(self, o: Any) -> "Col":
        return self._bin(o, _op.and_)

    def __or__(self, o: Any) -> "Col":
        return self._bin(o, _op.or_)

    def __invert__(self) -> "Col":
        raise NotImplementedError  # same as the reference (sql.py:44-45)

    def __hash__(self) -> int:
        return hash((type(self).__name__, self.name))

    def like(self, pattern: str) -> "Col":
        return LikeColumn(self, pattern)

    def between(self, start: Any, end: Any) -> "Col":
        # (start <= self) & (self <= end), written so that a plain-string bound works too
        return (self >= start) & (self <= end)

    def alias(self, name: str) -> "Col":
        return AliasColumn(self, name)

    def asc(self) -> "SortKey":
        return SortKey(self, True)

    def desc(self) -> "SortKey":
        return SortKey(self, False)

    # -- tree protocol ---------------------------------------------------------------------------------
    @property
    def children(self) -> tuple["Col", ...]:
        return ()

    @property
    def all_nested_columns(self) -> Iterator["Col"]:
        yield self
        for child in self.children:
            yield from child.all_nested_columns

    def normalize_agg_columns(self) -> "Col":
        return self

    def infer_type(self, schema: Schema) -> ColumnType:
        for col_name, col_type in schema:
            if col_name == self.name:
                return col_type
        raise ValueError(f'Column "{self.name}" not found in schema {schema}')

    def __str__(self) -> str:
        return self.name

    __repr__ = __str__


class SortKey:
    """``Col("a").asc()`` / ``.desc()``: one key of ``DataFrame.order_by`` (no reference counterpart - the reference has
    no ordering).  Not an expression: it cannot be selected, compared or nested."""

    def __init__(self, column: Col, ascending: bool) -> None:
        self.column, self.ascending = column, ascending

    def __str__(self) -> str:
        return f"{self.column} {'ASC' if self.ascending else 'DESC'}"

    __repr__ = __str__


class WindowItem:
    """``F.row_number() | F.rank() | F.dense_rank()`` ``.over(partition_by=[...], order_by=[...])`` ``[.alias(name)]``, or an
    aggregate ``F.sum(col) | F.avg(col) | F.min(col) | F.max(col) | F.count()`` ``.over(..., rows=False)``: one window column
    of ``DataFrame.window`` (no reference counterpart - DESIGN.md 4.4f, 4.4g).  The keys and an aggregate's argument are
    plain columns of the RESULT the window reads (``Col``, ``Col.asc()``, ``Col.desc()``).  A ranking item adds an INTEGER
    column named after its function; an aggregate item a column of ``out_type`` named as the aggregate is (``sum_v``,
    ``count``) - unless ``alias`` says otherwise.  ``frame`` (aggregates): "partition" - every row of the partition, no
    ORDER BY; "range" - through the row's last peer, the default with ORDER BY; "rows" - through the row itself
    (``rows=True``); "between" - ``rows=(n, m)``, ROWS BETWEEN n PRECEDING AND m FOLLOWING: the row's place
    j in its partition's order, the places ``[max(first, j - n), min(last, j + m)]``; ``preceding`` / ``following`` hold n and
    m (None for every other frame).  Not an expression: it cannot be selected, compared or nested.

    Navigation items: ``F.lag(col, offset, default) | F.lead(col, offset, default)`` - the value ``offset``
    rows before / after the row in its partition's order, ``default`` where the partition has no such row (both mandatory:
    there is no NULL); ``F.first_value(col) | F.last_value(col)`` - the value of the first / last row of the frame, the
    aggregates' frames; ``F.ntile(n)`` - the row's bucket of ``n``.  The value items copy cells of an INTEGER, FLOAT or
    TIMESTAMP column and have its type; NTILE is INTEGER.  Named ``lag_v``, ``lead_v``, ``first_value_v``, ``last_value_v``,
    ``ntile``."""

    RANKING = ("row_number", "rank", "dense_rank")
    AGGREGATES = ("sum", "avg", "min", "max", "count")
    NAVIGATION = ("lag", "lead", "first_value", "last_value", "ntile")
    KINDS = RANKING + AGGREGATES + NAVIGATION

    def __init__(self, kind: str, arg: Col | None = None, offset: Any = None, default: Any = None,
                 buckets: Any = None) -> None:
        if kind not in self.KINDS:
            raise ValueError(f"window function {kind!r}: one of {self.KINDS}")
        if kind in self.NAVIGATION:
            self._check_navigation(kind, arg, offset, default, buckets)
        elif (arg is not None) != (kind in self.AGGREGATES and kind != "count"):
            raise ValueError(f"window function {kind!r}: SUM / AVG / MIN / MAX take one column, every other function none")
        if arg is not None and type(arg).__name__ not in {"Col", "SchemaCol"}:
            raise ValueError(f"a window aggregate takes plain columns of the result, not the expression {arg}: "
                             "select(... .alias()) first")
        self.kind, self.arg = kind, arg
        self.offset, self.default, self.buckets = offset, default, buckets
        self.name = kind if arg is None else f"{kind}_{arg.name}"
        self.frame: str | None = None
        self.preceding: int | None = None
        self.following: int | None = None
        self.partition_by: list[Col] = []
        self.order_by: list[tuple[Col, bool]] = []
        self.is_over = False

    @staticmethod
    def _check_navigation(kind: str, arg: Any, offset: Any, default: Any, buckets: Any) -> None:
        whole = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
        head = kind.upper()
        if kind == "ntile":
            if arg is not None or offset is not None or default is not None:
                raise ValueError("NTILE(n) takes the number of buckets and nothing else")
            if not whole(buckets) or not 1 <= buckets < 1 << 31:
                raise ValueError(f"NTILE(n): n is an integer literal with 1 <= n < 2^31, not {buckets!r}")
            return
        if arg is None or buckets is not None:
            raise ValueError(f"window function {kind!r} takes one column of the result")
        if kind in ("first_value", "last_value"):
            if offset is not None or default is not None:
                raise ValueError(f"{head}(column) takes one column and nothing else")
            return
        shown = getattr(arg, "name", arg)
        if offset is None or default is None:
            raise ValueError(f"{head}: the offset k and the default are mandatory - there is no NULL to stand in for the row "
                             f"that does not exist, as CASE's ELSE is mandatory: write {head}({shown}, 1, 0)")
        if not whole(offset) or not 0 <= offset < 1 << 31:
            raise ValueError(f"{head}({shown}, k, default): k is an integer literal with 0 <= k < 2^31, not {offset!r}")
        if isinstance(default, bool) or not isinstance(default, (int, float, str)):
            raise ValueError(f"{head}({shown}, k, default): the default is a literal of the column's type (an integer, a "
                             f"number or a quoted ISO timestamp), not {default!r}")

    @staticmethod
    def _check_rows(rows: Any) -> tuple[int, int] | None:
        """``rows`` of ``over``: True / False -> None; (n, m) -> the pair, two integers in [0, 2^31); else ``ValueError``"""
        if isinstance(rows, bool):
            return None
        whole = lambda v: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 1 << 31  # noqa: E731
        if not isinstance(rows, (tuple, list)) or len(rows) != 2 or not all(whole(v) for v in rows):
            raise ValueError(f"rows= is True, False or a pair (n, m) of integers with 0 <= n, m < 2^31 - ROWS BETWEEN n PRECEDING "
                             f"AND m FOLLOWING - not {rows!r}")
        return int(rows[0]), int(rows[1])

    def over(self, partition_by: Any = (), order_by: Any = (), rows: Any = False) -> "WindowItem":
        between = self._check_rows(rows)
        single = lambda v: [v] if isinstance(v, (Col, SortKey)) else list(v)  # noqa: E731
        self.partition_by = single(partition_by)
        self.order_by = [(k.column, k.ascending) if isinstance(k, SortKey) else (k, True) for k in single(order_by)]
        for col in [*self.partition_by, *[c for c, _ in self.order_by]]:
            if type(col).__name__ not in {"Col", "SchemaCol"}:
                raise ValueError(f"OVER takes plain columns of the result, not the expression {col}: select(... .alias()) first")
        if self.kind in self.RANKING:
            if rows:
                raise ValueError(f"{self.kind.upper()}() takes no frame clause: a rank is a property of the row's place in its "
                                 "partition, not of a frame")
            if self.kind != "row_number" and not self.order_by:
                raise ValueError(f"{self.kind.upper()}() needs an ORDER BY inside OVER: without one every row of a partition is "
                                 "a peer of every other (ROW_NUMBER() may omit it)")
        elif self.kind in ("lag", "lead", "ntile"):
            if rows:
                raise ValueError(f"{self.kind.upper()}() takes no frame clause: it is a property of the row's place in its "
                                 "partition, not of a frame")
        elif between is not None:
            self.frame, (self.preceding, self.following) = "between", between
        else:
            self.frame = "rows" if rows else "range" if self.order_by else "partition"
            self.preceding = self.following = None
        self.is_over = True
        return self

    def alias(self, name: str) -> "WindowItem":
        self.name = name
        return self

    def spec(self) -> tuple:
        """What the sort depends on: items with one spec share one sort."""
        return (tuple(c.name for c in self.partition_by), tuple((c.name, asc) for c, asc in self.order_by))

    def out_type(self, schema: Schema) -> ColumnType:
        """The type of the column the item adds, given the schema of the rows it reads.  An aggregate's argument is an
        INTEGER or FLOAT column of them: ``TypeError`` that names it otherwise (a name the rows do not have: the ``ValueError``
        a key raises).  A navigation item's argument may be a TIMESTAMP column too, and the default of LAG / LEAD is a
        literal of the argument's type (``default_bits``)."""
        if self.arg is None:
            return ColumnType.INTEGER
        arg_type = self.arg.infer_type(schema)  # ValueError('Column "x" not found in schema ...')
        if self.kind in self.NAVIGATION:
            if arg_type not in (ColumnType.INTEGER, ColumnType.FLOAT, ColumnType.TIMESTAMP):
                raise TypeError(f'{self.kind.upper()}({self.arg.name}) OVER: column "{self.arg.name}" is {arg_type}; a window '
                                "navigation function takes an INTEGER, FLOAT or TIMESTAMP column")
            if self.kind in ("lag", "lead"):
                self.default_bits(arg_type)
            return arg_type
        if arg_type not in (ColumnType.INTEGER, ColumnType.FLOAT):
            raise TypeError(f'{self.kind.upper()}({self.arg.name}) OVER: column "{self.arg.name}" is {arg_type}; a window '
                            "aggregate takes an INTEGER or FLOAT column")
        return ColumnType.FLOAT if self.kind == "avg" else arg_type

    def default_bits(self, arg_type: ColumnType) -> int:
        """LAG / LEAD's default as the bits of a cell of ``arg_type``: an integer within i32 for INTEGER, a number rounded to
        a finite f32 for FLOAT, a quoted ISO timestamp for TIMESTAMP (microseconds, 8 bytes).  ``TypeError`` for a default
        of another type, ``OverflowError`` / ``ValueError`` for one the cell does not hold."""
        import struct  # noqa: PLC0415

        d, what = self.default, f'{self.kind.upper()}({self.arg.name}, {self.offset}, {self._shown_default()})'
        whole = isinstance(d, int) and not isinstance(d, bool)
        if arg_type == ColumnType.INTEGER:
            if not whole:
                raise TypeError(f'{what}: column "{self.arg.name}" is INTEGER, its default is an integer literal')
            if not -(1 << 31) <= d < 1 << 31:
                raise OverflowError(f"{what}: the default does not fit the 32 bits of an INTEGER cell")
            return d & 0xFFFFFFFF
        if arg_type == ColumnType.FLOAT:
            if not whole and not isinstance(d, float):
                raise TypeError(f'{what}: column "{self.arg.name}" is FLOAT, its default is a number literal')
            try:
                bits = struct.unpack("<I", struct.pack("<f", float(d)))[0]  # OverflowError beyond f32 (RNE inside)
            except OverflowError:
                raise OverflowError(f"{what}: the default does not fit a FLOAT cell (f32)") from None
            if bits & 0x7F800000 == 0x7F800000:
                raise ValueError(f"{what}: the default of a FLOAT column is a finite number")
            return bits
        if not isinstance(d, str):
            raise TypeError(f'{what}: column "{self.arg.name}" is TIMESTAMP, its default is a quoted ISO timestamp')
        from .utils import _timestamp_us  # noqa: PLC0415

        try:
            us = _timestamp_us(d)
        except ValueError:
            raise TypeError(f"{what}: the default of a TIMESTAMP column is a quoted ISO timestamp ('1970-01-01')") from None
        return us & 0xFFFFFFFFFFFFFFFF

    def _shown_default(self) -> str:
        return f"'{self.default}'" if isinstance(self.default, str) else str(self.default)

    def __str__(self) -> str:
        parts = []
        if self.partition_by:
            parts.append("PARTITION BY " + ", ".join(str(c) for c in self.partition_by))
        if self.order_by:
            parts.append("ORDER BY " + ", ".join(f"{c} {'ASC' if asc else 'DESC'}" for c, asc in self.order_by))
        if self.frame in ("rows", "range"):
            parts.append(f"{self.frame.upper()} UNBOUNDED PRECEDING")
        elif self.frame == "between":
            end = lambda k, side: f"{k} {side}" if k else "CURRENT ROW"  # noqa: E731
            parts.append(f"ROWS BETWEEN {end(self.preceding, 'PRECEDING')} AND {end(self.following, 'FOLLOWING')}")
        inner = "" if self.arg is None else str(self.arg)
        if self.kind in ("lag", "lead"):
            inner = f"{self.arg}, {self.offset}, {self._shown_default()}"
        elif self.kind == "ntile":
            inner = str(self.buckets)
        return f"{self.kind.upper()}({inner}) OVER ({' '.join(parts)}) AS {self.name}"

    __repr__ = __str__


class Lit(Col):
    def __init__(self, value: ColumnTypePython) -> None:
        self.value = value
        super().__init__(f"lit_{value}")

    def __hash__(self) -> int:
        return hash(("Lit", self.value))

    @property
    def all_nested_columns(self) -> Iterator[Col]:
        return iter(())

    def infer_type(self, schema: Schema) -> ColumnType:
        return ColumnType.of(self.value)

    def __str__(self) -> str:
        return str(self.value)

    __repr__ = __str__


class AliasColumn(Col):
    def __init__(self, original_col: Col, name: str) -> None:
        self.original_col = original_col
        super().__init__(name)

    def __hash__(self) -> int:
        return hash(("AliasColumn", hash(self.original_col), self.name))

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.original_col,)

    def infer_type(self, schema: Schema) -> ColumnType:
        return self.original_col.infer_type(schema)

    def __str__(self) -> str:
        return f"({self.original_col}) AS {self.name}"

    __repr__ = __str__


class LikeColumn(Col):
    """SQL LIKE: ``%`` = any run of characters, ``_`` = exactly one; anchored, case-sensitive.

    ``regex`` is kept for information (reference sql.py:178-179); the device matcher works on the
    pattern itself (no regex engine on the GPU)."""

    def __init__(self, original_col: Col, pattern: str) -> None:
        self.original_col = original_col
        self.pattern = pattern
        self.regex = "^" + re.escape(pattern).replace("%", ".*").replace("_", ".") + "$"
        super().__init__(f"{original_col.name}_like_{pattern}")

    def __hash__(self) -> int:
        return hash(("LikeColumn", hash(self.original_col), self.pattern))

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.original_col,)

    def infer_type(self, schema: Schema) -> ColumnType:
        if self.original_col.infer_type(schema) != ColumnType.STRING:
            raise AssertionError("LIKE operator can only be applied to string columns")
        return ColumnType.STRING  # the reference has no BOOL type (sql.py:202-205)

    def __str__(self) -> str:
        return f"({self.original_col}) LIKE '{self.pattern}'"

    __repr__ = __str__


class BinaryOperatorColumn(Col):
    def __init__(self, left_side: Any, right_side: Any, operator: Callable[..., Any]) -> None:
        self.left_side = _wrap(left_side)
        self.right_side = _wrap(right_side)
        self.operator = operator
        self.left_type_convert_to: ColumnType | None = None
        self.right_type_convert_to: ColumnType | None = None
        super().__init__(f"{self.left_side.name}_{operator.__name__}_{self.right_side.name}")

    def __hash__(self) -> int:
        return hash(("BinaryOperatorColumn", hash(self.left_side), hash(self.right_side), self.operator))

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.left_side, self.right_side)

    def infer_type(self, schema: Schema) -> ColumnType:
        """Promotion rules of the reference (sql.py:277-303): ``/`` is always FLOAT, INT op FLOAT is
        FLOAT, a string literal next to a TIMESTAMP is parsed as an ISO date (the literal node is
        rewritten in place), anything else must have equal operand types.  A comparison's type is its
        operands' type - there is no BOOL."""
        lt = self.left_side.infer_type(schema)
        rt = self.right_side.infer_type(schema)
        if self.operator is _op.truediv:
            self.left_type_convert_to = None if lt == ColumnType.FLOAT else ColumnType.FLOAT
            self.right_type_convert_to = None if rt == ColumnType.FLOAT else ColumnType.FLOAT
            return ColumnType.FLOAT
        if {lt, rt} == {ColumnType.INTEGER, ColumnType.FLOAT}:
            self.left_type_convert_to = ColumnType.FLOAT if lt == ColumnType.INTEGER else None
            self.right_type_convert_to = ColumnType.FLOAT if rt == ColumnType.INTEGER else None
            return ColumnType.FLOAT
        if lt == ColumnType.STRING and rt == ColumnType.TIMESTAMP:
            lt = self._literal_to_timestamp(self.left_side)
        if rt == ColumnType.STRING and lt == ColumnType.TIMESTAMP:
            rt = self._literal_to_timestamp(self.right_side)
        if lt != rt:
            raise TypeError(f"Type mismatch in binary operation: {lt} {self.operator} {rt}")
        return lt

    @staticmethod
    def _literal_to_timestamp(side: Col) -> ColumnType:
        if type(side).__name__ != "Lit":
            raise AssertionError("only a literal can be converted to TIMESTAMP")
        side.value = datetime.fromisoformat(str(side.value))  # type: ignore[attr-defined]
        return ColumnType.TIMESTAMP

    def normalize_agg_columns(self) -> Col:
        return BinaryOperatorColumn(
            self.left_side.normalize_agg_columns(), self.right_side.normalize_agg_columns(), self.operator
        )

    def extract_left_right_key(self, left_schema: Schema, right_schema: Schema) -> tuple[Col, Col]:
        """Which side of an equi-join condition belongs to which input (reference sql.py:343-355)."""
        a, b = self.left_side, self.right_side
        if type(a) is not Col or type(b) is not Col:
            raise AssertionError("join keys must be plain columns")
        if a.name == b.name:
            raise AssertionError("Join keys must be different columns")
        left_names = {n for n, _ in left_schema}
        right_names = {n for n, _ in right_schema}
        if a.name in left_names and b.name in right_names:
            return a, b
        if a.name in right_names and b.name in left_names:
            return b, a
        raise ValueError("Join keys must be from different tables")

    def __str__(self) -> str:
        return f"({self.left_side}) {BINOP_SYMBOLS[self.operator]} ({self.right_side})"

    __repr__ = __str__


_BOOLEAN_OPERATORS = (_op.eq, _op.ne, _op.lt, _op.le, _op.gt, _op.ge, _op.and_, _op.or_)


def _is_boolean(node: Col) -> bool:
    """A comparison, AND / OR, LIKE or a bool literal: there is no BOOL column type, so the node's shape decides."""
    while isinstance(node, AliasColumn):
        node = node.original_col
    if isinstance(node, BinaryOperatorColumn):
        return node.operator in _BOOLEAN_OPERATORS
    return isinstance(node, LikeColumn) or (isinstance(node, Lit) and type(node.value) is bool)


class CaseColumn(Col):
    """``CASE WHEN condition THEN then_col ELSE else_col END`` (no reference counterpart: DESIGN.md 4.4b).  Several WHEN
    arms nest to the right in ``else_col``.  Both branches are numeric; the value is FLOAT if either is.  Both branches
    are evaluated for every surviving row, then one is chosen (an error inside the branch not taken is still raised)."""

    def __init__(self, condition: Any, then_col: Any, else_col: Any) -> None:
        self.condition = _wrap(condition)
        self.then_col = _wrap(then_col)
        self.else_col = _wrap(else_col)
        super().__init__(f"case_{self.condition.name}_then_{self.then_col.name}_else_{self.else_col.name}")

    def __hash__(self) -> int:
        return hash(("CaseColumn", hash(self.condition), hash(self.then_col), hash(self.else_col)))

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.condition, self.then_col, self.else_col)

    def infer_type(self, schema: Schema) -> ColumnType:
        self.condition.infer_type(schema)
        types = []
        for branch in (self.then_col, self.else_col):
            branch_type = branch.infer_type(schema)
            if branch_type not in (ColumnType.INTEGER, ColumnType.FLOAT) or _is_boolean(branch):
                what = "boolean" if _is_boolean(branch) else branch_type.name
                raise TypeError(f"CASE branches are INTEGER or FLOAT values, not {what}: {branch} in {self}")
            types.append(branch_type)
        return ColumnType.FLOAT if ColumnType.FLOAT in types else ColumnType.INTEGER

    def normalize_agg_columns(self) -> Col:
        return CaseColumn(self.condition.normalize_agg_columns(), self.then_col.normalize_agg_columns(),
                          self.else_col.normalize_agg_columns())

    def _arms(self) -> str:
        tail = self.else_col
        rest = tail._arms() if type(tail) is CaseColumn else f"ELSE {tail} END"
        return f"WHEN {self.condition} THEN {self.then_col} {rest}"

    def __str__(self) -> str:
        return f"CASE {self._arms()}"

    __repr__ = __str__


DATE_PARTS = ("year", "quarter", "month", "day", "hour", "minute", "second", "dayofweek", "dayofyear")
DATE_TRUNC_UNITS = ("year", "quarter", "month", "week", "day", "hour", "minute", "second")


class _DateFunctionColumn(Col):
    """What the two date functions share (no reference counterpart: DESIGN.md 4.4d): one TIMESTAMP-valued argument - a
    TIMESTAMP column, a ``datetime`` literal or a DATE_TRUNC - read in the proleptic Gregorian calendar without a time
    zone.  The functions are total: they raise on no value of the column."""

    _WORDS: tuple[str, ...] = ()
    _KIND = ""

    def __init__(self, word: str, col: Any) -> None:
        if not isinstance(word, str) or word.lower() not in self._WORDS:
            raise ValueError(f"{self._KIND} {word!r}: one of {', '.join(self._WORDS)}")
        self.original_col = _wrap(col)
        self._word = word.lower()
        super().__init__(f"{self._prefix()}_{self.original_col.name}")

    def _prefix(self) -> str:
        raise NotImplementedError

    def __hash__(self) -> int:
        return hash((type(self).__name__, self._word, hash(self.original_col)))

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.original_col,)

    def _check_argument(self, schema: Schema) -> None:
        arg_type = self.original_col.infer_type(schema)
        if arg_type != ColumnType.TIMESTAMP:
            raise TypeError(f"{self}: the argument of a date function is a TIMESTAMP value, not {arg_type.name}")

    def normalize_agg_columns(self) -> Col:
        return type(self)(self._word, self.original_col.normalize_agg_columns())


class DatePartColumn(_DateFunctionColumn):
    """``YEAR(ts)`` ... ``DAYOFYEAR(ts)``: an INTEGER.  QUARTER 1-4, MONTH 1-12, DAY 1-31, HOUR 0-23, MINUTE and SECOND
    0-59 (whole seconds), DAYOFWEEK in ISO numbering (Monday 1 ... Sunday 7), DAYOFYEAR 1-366; division is floor division,
    so the microsecond before 1970 has year 1969, day 31, hour 23."""

    _WORDS, _KIND = DATE_PARTS, "date part"

    def __init__(self, part: str, col: Any) -> None:
        super().__init__(part, col)
        self.part = self._word

    def _prefix(self) -> str:
        return self._word

    def infer_type(self, schema: Schema) -> ColumnType:
        self._check_argument(schema)
        return ColumnType.INTEGER

    def __str__(self) -> str:
        return f"{self.part.upper()}({self.original_col})"

    __repr__ = __str__


class DateTruncColumn(_DateFunctionColumn):
    """``DATE_TRUNC('unit', ts)``: the first microsecond of the unit that holds ``ts``, a TIMESTAMP; a week starts on
    Monday."""

    _WORDS, _KIND = DATE_TRUNC_UNITS, "DATE_TRUNC unit"

    def __init__(self, unit: str, col: Any) -> None:
        super().__init__(unit, col)
        self.unit = self._word

    def _prefix(self) -> str:
        return f"date_trunc_{self._word}"

    def infer_type(self, schema: Schema) -> ColumnType:
        self._check_argument(schema)
        return ColumnType.TIMESTAMP

    def __str__(self) -> str:
        return f"DATE_TRUNC('{self.unit}', {self.original_col})"

    __repr__ = __str__


class KeyTupleCol(Col):
    """The key of a GROUP BY over several columns (no reference counterpart: DESIGN.md 4.4c): ``parts`` are plain columns
    of the aggregate's input, in the order given.  Between the partial aggregate and the final merge the tuple travels as
    ONE column of fixed-width bytes under this node's reserved name - parentheses and commas, which no column the parser
    reads can carry - so its type is STRING; ``packed`` marks the nodes of the physical plan that see that column, the
    logical aggregate (``packed`` False) yields the parts themselves."""

    MAX_PARTS = 8

    def __init__(self, parts: Iterable[Col], packed: bool = False) -> None:
        self.parts = tuple(parts)
        self.packed = packed
        super().__init__("__hs_key(" + ",".join(p.name for p in self.parts) + ")")

    def __hash__(self) -> int:
        return hash(("KeyTupleCol", tuple(hash(p) for p in self.parts)))

    @property
    def children(self) -> tuple[Col, ...]:
        return self.parts

    def as_packed(self) -> "KeyTupleCol":
        return KeyTupleCol(self.parts, packed=True)

    def part_schema(self, schema: Schema) -> Schema:
        return [(p.name, p.infer_type(schema)) for p in self.parts]

    def infer_type(self, schema: Schema) -> ColumnType:
        if not any(name == self.name for name, _ in schema):  # (behind the partial aggregate only the packed column is left)
            self.part_schema(schema)  # ValueError('Column "x" not found in schema ...')
        return ColumnType.STRING

    def __str__(self) -> str:
        return "(" + ", ".join(str(p) for p in self.parts) + ")"

    __repr__ = __str__


# instance fields of the column classes that code reads without calling anything
_COL_FIELDS = frozenset({"name", "original_col", "left_side", "right_side", "operator", "value", "pattern", "type",
                         "condition", "then_col", "else_col", "part", "unit"})


class CaseBuilder:
    """``Functions.when(cond, value)[.when(cond, value)...]``: unfinished until ``.otherwise(value)`` (ELSE is mandatory:
    the data model has no NULL).  Not a column."""

    def __init__(self, arms: list[tuple[Any, Any]]) -> None:
        self._arms = arms

    def when(self, condition: Any, value: Any) -> "CaseBuilder":
        return CaseBuilder([*self._arms, (condition, value)])

    def otherwise(self, value: Any) -> CaseColumn:
        col = _wrap(value)
        for condition, then in reversed(self._arms):
            col = CaseColumn(condition, then, col)
        return col  # type: ignore[return-value]

    def _unfinished(self, *args: Any, **kwargs: Any) -> Any:
        raise TypeError("CASE without ELSE: finish Functions.when(...) with .otherwise(value) before using it as a column")

    def __getattr__(self, name: str) -> Any:
        # only what a column is asked for: hasattr() / getattr(builder, name, default) of anything else answer as usual
        if not name.startswith("__") and hasattr(Col, name) or name in _COL_FIELDS:
            self._unfinished()
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    __add__ = __radd__ = __sub__ = __mul__ = __truediv__ = __floordiv__ = __mod__ = _unfinished
    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = __and__ = __or__ = _unfinished  # type: ignore[assignment]
    __hash__ = None  # type: ignore[assignment]


class AggCol(Col):
    """``type`` in {"sum","min","max","avg"} applied to ``original_col`` (reference sql.py:399-446), or
    ``"count_distinct"`` (no reference counterpart: DESIGN.md 4.4e), the number of different values of ``original_col``,
    an INTEGER; the planner carries it as the SUM of a first-occurrence mark column (``MarkFirstTask``)."""

    def __init__(self, agg_type: str, original_col: Col) -> None:
        self.original_col = original_col
        self.type = agg_type
        super().__init__(f"{agg_type}_{original_col.name}")

    def __hash__(self) -> int:
        return hash(("AggCol", self.type, hash(self.original_col), self.name))

    def alias(self, name: str) -> "AggCol":  # renames in place and stays an AggCol (sql.py:421-423)
        self.name = name
        return self

    @property
    def children(self) -> tuple[Col, ...]:
        return (self.original_col,)

    def infer_type(self, schema: Schema) -> ColumnType:
        if self.type == "count_distinct":
            self.original_col.infer_type(schema)  # ValueError('Column "x" not found in schema ...')
            return ColumnType.INTEGER
        return ColumnType.FLOAT if self.type == "avg" else self.original_col.infer_type(schema)

    def normalize_agg_columns(self) -> Col:
        return Col(self.name)

    def over(self, partition_by: Any = (), order_by: Any = (), rows: Any = False) -> WindowItem:
        """The aggregate as a window item: ``F.sum(Col("v")).over(partition_by=[Col("k")])``; it keeps the
        aggregate's name.  ``F.count().over(...)`` counts the frame's rows.  ``rows=True``: ROWS UNBOUNDED PRECEDING;
        ``rows=(n, m)``: ROWS BETWEEN n PRECEDING AND m FOLLOWING (4.4i)."""
        if self.type == "count_distinct":
            raise ValueError(f"{self}: COUNT(DISTINCT) has no window form")
        arg = self.original_col
        if self.type == "sum" and type(arg) is Lit and arg.value == 1:
            item = WindowItem("count")
        else:
            item = WindowItem(self.type, arg)
        return item.alias(self.name).over(partition_by=partition_by, order_by=order_by, rows=rows)

    def expand_avg(self) -> Iterable["AggCol"]:
        """AVG(x) is carried through the shuffle as SUM(x) and SUM(1) (sql.py:436-441)."""
        if self.type != "avg":
            return [self]
        return [
            AggCol("sum", self.original_col).alias(f"{self.name}_sum"),
            AggCol("sum", Lit(1)).alias(f"{self.name}_count"),
        ]

    def projection(self) -> Col:
        if self.type == "avg":
            return (Col(f"{self.name}_sum") / Col(f"{self.name}_count")).alias(self.name)
        return Col(self.name)

    def __str__(self) -> str:
        return f"{self.type}({self.original_col}) AS {self.name}"

    __repr__ = __str__


class Functions:
    @staticmethod
    def min(col: Col) -> AggCol:
        return AggCol("min", col)

    @staticmethod
    def max(col: Col) -> AggCol:
        return AggCol("max", col)

    @staticmethod
    def sum(col: Col) -> AggCol:
        return AggCol("sum", col)

    @staticmethod
    def avg(col: Col) -> AggCol:
        return AggCol("avg", col)

    @staticmethod
    def count() -> AggCol:
        return AggCol("sum", Lit(1)).alias("count")

    @staticmethod
    def count_distinct(col: Col) -> AggCol:
        """COUNT(DISTINCT col): the number of different values of ``col`` (a column, or an INTEGER / FLOAT / TIMESTAMP
        valued expression) among the rows of the group; named ``count_distinct_<name>``."""
        return AggCol("count_distinct", _wrap(col))

    # window ranking (WindowItem): DESIGN.md 4.4f
    @staticmethod
    def row_number() -> WindowItem:
        return WindowItem("row_number")

    @staticmethod
    def rank() -> WindowItem:
        return WindowItem("rank")

    @staticmethod
    def dense_rank() -> WindowItem:
        return WindowItem("dense_rank")

    # window navigation: DESIGN.md 4.4h
    @staticmethod
    def lag(col: Col, offset: Any = None, default: Any = None) -> WindowItem:
        return WindowItem("lag", col, offset=offset, default=default)

    @staticmethod
    def lead(col: Col, offset: Any = None, default: Any = None) -> WindowItem:
        return WindowItem("lead", col, offset=offset, default=default)

    @staticmethod
    def first_value(col: Col) -> WindowItem:
        return WindowItem("first_value", col)

    @staticmethod
    def last_value(col: Col) -> WindowItem:
        return WindowItem("last_value", col)

    @staticmethod
    def ntile(n: int) -> WindowItem:
        return WindowItem("ntile", buckets=n)

    @staticmethod
    def when(condition: Any, value: Any) -> CaseBuilder:
        """``when(c, x).otherwise(y)`` = CASE WHEN c THEN x ELSE y END; further ``.when`` arms nest to the right."""
        return CaseBuilder([(condition, value)])

    # date parts of a TIMESTAMP value (DatePartColumn) and DATE_TRUNC (DateTruncColumn): DESIGN.md 4.4d
    @staticmethod
    def year(col: Any) -> DatePartColumn:
        return DatePartColumn("year", col)

    @staticmethod
    def quarter(col: Any) -> DatePartColumn:
        return DatePartColumn("quarter", col)

    @staticmethod
    def month(col: Any) -> DatePartColumn:
        return DatePartColumn("month", col)

    @staticmethod
    def day(col: Any) -> DatePartColumn:
        return DatePartColumn("day", col)

    @staticmethod
    def hour(col: Any) -> DatePartColumn:
        return DatePartColumn("hour", col)

    @staticmethod
    def minute(col: Any) -> DatePartColumn:
        return DatePartColumn("minute", col)

    @staticmethod
    def second(col: Any) -> DatePartColumn:
        return DatePartColumn("second", col)

    @staticmethod
    def dayofweek(col: Any) -> DatePartColumn:
        return DatePartColumn("dayofweek", col)

    @staticmethod
    def dayofyear(col: Any) -> DatePartColumn:
        return DatePartColumn("dayofyear", col)

    @staticmethod
    def date_trunc(unit: str, col: Any) -> DateTruncColumn:
        return DateTruncColumn(unit, col)
