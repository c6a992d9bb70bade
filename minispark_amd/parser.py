"""SQL text -> DataFrame (reference: src/mini_spark/parser.py - the grammar at :14-69 and what its visitor builds
at :124-162; the reference parses with the third-party `parsimonious`, which is not part of this package's
requirements, so `.sql()` would not work next to the HIP engine without this module).

A hand-written backtracking recursive-descent parser for the same language:

    SELECT [DISTINCT] select_list FROM 'path' [AS t] { [LEFT|RIGHT|INNER|FULL] JOIN 'path' [AS t] ON cond
                                                       | [LEFT] SEMI JOIN 'path' [AS t] ON cond | [LEFT] ANTI JOIN 'path' [AS t] ON cond }
           [WHERE cond] [GROUP BY col | (col {, col}) [HAVING cond]] [ORDER BY name [ASC|DESC] {, name [ASC|DESC]}] [LIMIT n] ;

* select items: ``*``, ``COUNT()/SUM(e)/AVG(e)/MIN(e)/MAX(e)/COUNT(DISTINCT e) [AS name]``, ``expr [AS name]``;
* conditions: OR < AND < NOT < comparison | ( cond ) | BETWEEN | LIKE, comparators = != <= >= < >;
* expressions: + - over * / over atoms (number, column, string literal, ( expr ), COUNT()/SUM(e),
  ``CASE WHEN cond THEN expr {WHEN cond THEN expr} ELSE expr END``, the date functions ``YEAR(e)`` ``QUARTER(e)``
  ``MONTH(e)`` ``DAY(e)`` ``HOUR(e)`` ``MINUTE(e)`` ``SECOND(e)`` ``DAYOFWEEK(e)`` ``DAYOFYEAR(e)`` and
  ``DATE_TRUNC('unit', e)`` over a TIMESTAMP value; any other function name is a ``SemanticError``);
* a name in GROUP BY that is the alias of a select item made of one date-function call groups by that item
  (``SELECT YEAR(d) AS y, SUM(x) AS s FROM 't' GROUP BY y;``): the parser projects the item under its alias, next to the
  other keys and the plain columns the aggregates read, and groups by the projected column;
* a select list of aggregate calls only and no GROUP BY aggregates the whole table (``DataFrame.agg``): one row, or none
  when no row survives the WHERE; mixing aggregates and plain columns without GROUP BY raises ``GroupByError``, HAVING
  without GROUP BY stays a syntax error, arithmetic over aggregates (``SUM(a) / SUM(b)``) is not part of this form;
* like the reference: whitespace is required around keywords, the closing ``;`` is mandatory, every join kind
  is executed as an inner join (parser.py:131-133), numbers are integers (parser.py:349), NOT raises
  NotImplementedError (sql.py:44-45), the unparenthesised GROUP BY takes one column (dataframe.py:64);
* beyond the reference: ORDER BY takes names of the RESULT (a select item's alias, or its generated name), each ascending
  unless DESC follows, and LIMIT a non-negative integer; both become one ``order_by`` / ``limit`` after the final select;
  ``SELECT DISTINCT`` (the keyword, then whitespace) becomes ``distinct()`` between the final select and ``order_by``:
  rows equal in every result column are removed, the first of them stays, and ORDER BY / LIMIT apply to what is left.
  The form without the keyword is tried first, so a text that was accepted before builds the tree it built then.
* window ranking, aggregates and navigation, tried only after every older form failed, so accepted texts keep their trees:
      select item:  ROW_NUMBER() | RANK() | DENSE_RANK()  OVER ( [PARTITION BY name {, name}]
                                                                 [ORDER BY name [ASC|DESC] {, name [ASC|DESC]}] )  [AS alias]
                    SUM(name) | AVG(name) | MIN(name) | MAX(name) | COUNT()  OVER ( [PARTITION BY ...] [ORDER BY ...] [frame] )
                    frame:  ROWS | RANGE  [BETWEEN]  UNBOUNDED PRECEDING  [AND CURRENT ROW]         [AS alias]
                         |  ROWS BETWEEN (n PRECEDING | CURRENT ROW) AND (m FOLLOWING | CURRENT ROW)
                            (n, m: integer literals below 2^31; BETWEEN mandatory, both ends finite:
                            ROWS 3 PRECEDING, an UNBOUNDED end next to a finite one, GROUPS and a RANGE of values stay
                            syntax errors)
                    LAG(name, k, default) | LEAD(name, k, default) | NTILE(n)  OVER ( [PARTITION BY ...] [ORDER BY ...] )
                    FIRST_VALUE(name) | LAST_VALUE(name)  OVER ( [PARTITION BY ...] [ORDER BY ...] [frame] )   [AS alias]
                    (k, n: integer literals; default: an integer, a decimal - either may be negative -
                    or a quoted ISO timestamp, of the column's type; k and default are mandatory: there is no NULL)
      clause:       ... [GROUP BY ... [HAVING ...]] [QUALIFY cond] [ORDER BY ...] [LIMIT n] ;
  The items are set aside from the select list (before GROUP BY's stray-column check), the rest of the query is built as
  ever, and ``window(...)`` / ``qualify(cond)`` follow the final select; names inside OVER are names of the RESULT, as for
  ORDER BY.  ``ROW_NUMBER()`` without OVER, ``RANK(x)`` and ``LAG(x)`` without OVER stay the unsupported functions they were.
  ``CASE`` (searched form only, ELSE mandatory, INTEGER / FLOAT branches, several WHEN arms nest to the right) stands
  wherever an expression may: a select item, an aggregate's argument, either side of a comparison, inside arithmetic or
  another CASE.  A column called ``CASE`` still parses as a column (no old text holds ``CASE`` whitespace ``WHEN``).

* GROUP BY over several columns is spelled in the row form, ``GROUP BY (a, b {, c})``: parentheses around a comma list of
  up to eight plain columns, optional whitespace inside; it becomes ``group_by(a, b, ...)`` and the result holds the key
  columns under their own names.  ``GROUP BY (a)`` is ``GROUP BY a``.  The row form is tried after the
  bare column, so every text accepted before builds the tree it built.  The unparenthesised list ``GROUP BY a, b`` is
  still rejected with a ``TypeError`` (its message points at the row form): tests/test_parser.py pins that rejection.

* ``COUNT(DISTINCT e)`` - the keyword, whitespace, exactly one expression - is ``Functions.count_distinct(e)``: the number
  of different values of ``e`` in the group, as a select item and inside HAVING.  It is tried after the
  forms above, so ``COUNT(DISTINCT)`` still reads a column called DISTINCT and raises what it raised, and every text
  accepted before builds the tree it built.  ``COUNT(DISTINCT a, b)`` and ``SUM(DISTINCT a)`` are not part of the language.

* ``[LEFT] SEMI JOIN 'path' [AS t] ON cond`` / ``[LEFT] ANTI JOIN ...`` keep the rows of the query so far
  that have / lack a partner in the table: ``join(other, on, how="left_semi" | "left_anti")``.  ``cond`` is one equality
  between a column of each side, optionally AND-ed with conditions over the joined table's columns (``ON o_orderkey =
  l_orderkey AND l_quantity > 45``).  The result keeps the left side's columns only, so the joined table's columns are
  unknown names to everything after it.  Joins apply left to right: ``A JOIN B ON ... LEFT ANTI JOIN C ON ...`` filters the
  join's rows.  The four spellings are tried after the five join kinds above, which keep running as the inner join.

Alternatives are tried in the grammar's order and the first that fits wins (ordered choice), so texts the
reference accepts build the same task tree here (tests/test_parser.py compares both renderings).
"""

from __future__ import annotations

import operator
import re
from typing import Any, Callable

from .dataframe import DataFrame
from .sql import (DATE_PARTS, AggCol, AliasColumn, CaseColumn, Col, DatePartColumn, DateTruncColumn, Lit, SortKey,
                  WindowItem)
from .sql import Functions as F


class SqlSyntaxError(ValueError):
    """The text is not a query of the supported language (the reference raises parsimonious' ParseError)."""


class SemanticError(Exception):
    pass


class GroupByError(SemanticError):
    pass


class _NoMatch(Exception):
    pass


_WS = re.compile(r"\s+")
_TABLE = re.compile(r"[a-zA-Z0-9_\-\./ ]+")
_COLUMN = re.compile(r"[A-Za-z_][A-Za-z0-9_\.]*")
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*")
_IDENT_CHAR = re.compile(r"[A-Za-z0-9_]")
_NUMBER = re.compile(r"-?[0-9]+(\.[0-9]+)?")
_DIGITS = re.compile(r"[0-9]+")
_STRING = re.compile(r"[^']*")
_COMPARATORS: list[tuple[str, Callable[[Any, Any], Any]]] = [
    ("=", operator.eq), ("!=", operator.ne), ("<=", operator.le), (">=", operator.ge), ("<", operator.lt),
    (">", operator.gt),
]
_JOIN_KINDS = [("JOIN",), ("LEFT", "JOIN"), ("RIGHT", "JOIN"), ("INNER", "JOIN"), ("FULL", "JOIN")]
_SEMI_JOIN_KINDS = [(("SEMI", "JOIN"), "left_semi"), (("LEFT", "SEMI", "JOIN"), "left_semi"),
                    (("ANTI", "JOIN"), "left_anti"), (("LEFT", "ANTI", "JOIN"), "left_anti")]
_AGGREGATES = ("COUNT", "SUM", "AVG", "MIN", "MAX")
_NAVIGATION = ("LAG", "LEAD", "FIRST_VALUE", "LAST_VALUE", "NTILE")


class _Parser:
    def __init__(self, text: str, engine: Any) -> None:
        self.text, self.pos, self.engine = text, 0, engine
        self.furthest = 0
        self.saw_window_item = False

    # ---- matching primitives --------------------------------------------------------------------------------
    def fail(self) -> None:
        self.furthest = max(self.furthest, self.pos)
        raise _NoMatch

    def lit(self, s: str) -> str:
        if not self.text.startswith(s, self.pos):
            self.fail()
        self.pos += len(s)
        return s

    def rx(self, pattern: re.Pattern) -> str:
        m = pattern.match(self.text, self.pos)
        if m is None or m.end() == m.start():
            self.fail()
        self.pos = m.end()
        return m.group(0)

    def ws(self) -> None:
        self.rx(_WS)

    def ows(self) -> None:
        m = _WS.match(self.text, self.pos)
        if m:
            self.pos = m.end()

    def attempt(self, rule: Callable[[], Any]) -> tuple[bool, Any]:
        start = self.pos
        try:
            return True, rule()
        except _NoMatch:
            self.pos = start
            return False, None

    def first_of(self, *rules: Callable[[], Any]) -> Any:
        for rule in rules:
            ok, value = self.attempt(rule)
            if ok:
                return value
        self.fail()
        return None

    def repeat(self, rule: Callable[[], Any]) -> list[Any]:
        out = []
        while True:
            ok, value = self.attempt(rule)
            if not ok:
                return out
            out.append(value)

    # ---- query ------------------------------------------------------------------------------------------------
    def query(self) -> DataFrame:
        # ordered choice: the grammar without DISTINCT first, so a text that was accepted before DISTINCT existed (a
        # column may be called DISTINCT) still builds the tree it built then
        # ... and the grammar without window items and QUALIFY before the one with them.  The older grammar answers a
        # window item with an exception (ROW_NUMBER is an unsupported function to it), so that exception is kept and
        # raised again when the text is no windowed query either
        try:
            matched, df = self.attempt(lambda: self.query_body(distinct=False))
            if matched:
                return df
            return self.query_body(distinct=True)
        except _NoMatch:
            before: Exception | None = None
        except Exception as exc:  # noqa: BLE001 - whatever the older grammar raised is raised again below
            before = exc
        self.pos = 0
        matched, df = self.attempt(lambda: self.query_body(distinct=False, windowed=True))
        if not matched:
            matched, df = self.attempt(lambda: self.query_body(distinct=True, windowed=True))
        if matched:
            return df
        if before is not None and not self.saw_window_item:
            raise before
        self.fail()  # a text with a well-formed window item that is no query: a syntax error at the furthest offset
        return None

    def query_body(self, distinct: bool, windowed: bool = False) -> DataFrame:
        self.ows()
        self.lit("SELECT")
        self.ws()
        if distinct:
            self.lit("DISTINCT")
            self.ws()
        select_list = self.select_list(windowed)
        self.ws()
        self.lit("FROM")
        self.ws()
        df = self.table_reference()
        joins = self.repeat(lambda: (self.ws(), self.join_clause())[1])
        has_where, where = self.attempt(lambda: (self.ws(), self.where_clause())[1])
        has_group, group = self.attempt(lambda: (self.ws(), self.group_by_clause())[1])
        has_qualify, qualify = self.attempt(lambda: (self.ws(), self.qualify_clause())[1]) if windowed else (False, None)
        has_order, order = self.attempt(lambda: (self.ws(), self.order_by_clause())[1])
        has_limit, limit = self.attempt(lambda: (self.ws(), self.limit_clause())[1])
        self.ows()
        self.lit(";")
        self.ows()
        if self.pos != len(self.text):
            self.fail()
        # window items are set aside: they read the rows the rest of the query produces
        result_list = select_list
        windows = [c for c in select_list if type(c) is WindowItem]
        select_list = [c for c in select_list if type(c) is not WindowItem]
        if windowed:
            if not windows and not has_qualify:
                self.fail()  # no windowed query: what the older grammar said about the text stands
            if not windows:
                raise SemanticError("QUALIFY filters on window columns: the select list has no window item")
            if not select_list:
                raise SemanticError("a select list needs at least one column next to its window items")

        for other, cond, how in joins:  # left to right: a semi / anti join filters the rows of the joins before it
            df = df.join(other, on=cond, how=how)
        if has_where:
            df = df.filter(where)
        if has_group:
            group_cols, having, row_form = group
            if len(group_cols) > 1 and not row_form:
                raise TypeError(f"GROUP BY {', '.join(c.name for c in group_cols)}: a bare GROUP BY takes one column; "
                                f"write the row form GROUP BY ({', '.join(c.name for c in group_cols)}) for several")
            key_names = {c.name for c in group_cols}
            agg_cols = [c for c in select_list if type(c) is AggCol]
            stray = [c for c in select_list if type(c) is not AggCol and c.name not in key_names]
            if stray:
                raise GroupByError(
                    "All selected columns must be aggregate functions or part of the key when using GROUP BY:\n"
                    f"{stray}"
                )
            if having is not None:
                extra = [c for c in having.all_nested_columns if type(c) is AggCol]
                for c in extra:
                    c.name = f"_having_{c.name}"
                agg_cols.extend(extra)
            df = self.project_date_keys(df, select_list, group_cols, agg_cols)
            df = df.group_by(*group_cols).agg(*agg_cols)
            if having is not None:
                df = df.filter(having.normalize_agg_columns())
            df = df.select(*[Col(c.name) for c in select_list])
        elif any(type(c) is AggCol for c in select_list):
            stray = [c for c in select_list if type(c) is not AggCol]
            if stray:
                raise GroupByError(
                    "Without GROUP BY a select list holds either aggregate functions only or none at all:\n"
                    f"{stray}"
                )
            df = df.agg(*select_list)
        else:
            df = df.select(*select_list)
        if windows:
            names = [c.name for c in result_list]
            trailing = all(type(c) is WindowItem for c in result_list[len(select_list):])
            if not trailing and "*" in names:
                raise SemanticError("next to * the window items come last in the select list")
            df = df.window(*windows, select_order=None if trailing else names)
            if has_qualify:
                df = df.qualify(qualify)
        if distinct:
            df = df.distinct()
        if has_order:
            names = {c.name for c in result_list}
            for key in order:
                if "*" not in names and key.column.name not in names:
                    raise ValueError(f'Column "{key.column.name}" of ORDER BY is not in the select list {sorted(names)}')
            df = df.order_by(*order)
        if has_limit:
            df = df.limit(limit)
        return df

    @staticmethod
    def project_date_keys(df: DataFrame, select_list: list[Col], group_cols: list[Col], agg_cols: list[AggCol]) -> DataFrame:
        """GROUP BY on the alias of a select item that is a date-function call (``SELECT YEAR(d) AS y, ... GROUP BY y``): the
        DataFrame idiom for a computed key - a projection of that item under its alias, the other keys and every plain
        column the aggregates (HAVING's among them) read, in front of the group_by.  Limited to date-function items: for any
        other aliased item the text parsed before these functions existed and keeps its tree."""
        items = {c.name: c for c in select_list
                 if type(c) is AliasColumn and type(c.original_col) in (DatePartColumn, DateTruncColumn)}
        if not any(g.name in items for g in group_cols):
            return df
        columns: list[Col] = [items.get(g.name, g) for g in group_cols]
        names = [c.name for c in columns]
        for agg in agg_cols:
            for c in agg.all_nested_columns:
                if type(c) is Col and c.name in items:
                    raise ValueError(f'"{c.name}" names a date function of the select list and is read by {agg} as a column')
                if type(c) is Col and c.name not in names:
                    names.append(c.name)
                    columns.append(Col(c.name))
        return df.select(*columns)

    def select_list(self, windowed: bool = False) -> list[Any]:
        item = self.select_item_or_window if windowed else self.select_item
        items = [item()]
        items += self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), item())[3])
        return items

    def select_item_or_window(self) -> Any:
        return self.first_of(self.star, self.window_item, self.aggregate_call, self.expr_aliased)

    def window_item(self) -> WindowItem:
        """ROW_NUMBER() | RANK() | DENSE_RANK() | SUM(name) | AVG(name) | MIN(name) | MAX(name) | COUNT() |
        LAG(name, k, default) | LEAD(name, k, default) | FIRST_VALUE(name) | LAST_VALUE(name) | NTILE(n), whitespace,
        OVER ( [PARTITION BY names] [ORDER BY keys] [frame] ) [AS alias].  Anything else - no OVER, an argument to a
        ranking function - is no window item and goes on to the function call it was before."""
        name = self.first_of(*[(lambda n=n: self.lit(n)) for n in ("ROW_NUMBER", "RANK", "DENSE_RANK", *_AGGREGATES,
                                                                  *_NAVIGATION)])
        ranking = name not in _AGGREGATES and name not in _NAVIGATION
        self.ows()
        self.lit("(")
        self.ows()
        arg = None
        extra: list[Any] = []  # LAG / LEAD: the literals behind the column; NTILE: its literal

        def literal() -> Any:
            """an integer, a decimal (either may be negative) or a quoted string"""
            has_number, text = self.attempt(lambda: self.rx(_NUMBER))
            if has_number:
                return float(text) if "." in text else int(text)
            return self.string_literal()

        if name == "NTILE":
            extra = [literal()]
            self.ows()
            self.lit(")")
        elif name in ("LAG", "LEAD"):
            def plain() -> Col:
                col = self.column_name()
                self.ows()
                if not self.text.startswith((",", ")"), self.pos):
                    self.fail()
                return col

            has_name, arg = self.attempt(plain)
            if not has_name:
                self.expr()
            extra = self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), literal())[3])
            self.ows()
            self.lit(")")
            if not has_name:  # as for an aggregate: a window item only if OVER follows
                self.ws()
                self.lit("OVER")
                raise SemanticError(f"{name}(...) OVER takes a plain column of the result, not an expression: alias the "
                                    f"expression in the select list (SELECT a + 1 AS x, {name}(x, 1, 0) OVER (...))")
        elif not ranking and name != "COUNT":
            has_name, arg = self.attempt(lambda: (self.column_name(), self.ows(), self.lit(")"))[0])
            if not has_name:  # an expression: a window item only if OVER follows, and then one that says what to do
                self.expr()
                self.ows()
                self.lit(")")
                self.ws()
                self.lit("OVER")
                raise SemanticError(f"{name}(...) OVER takes a plain column of the result, not an expression: alias the "
                                    f"expression in the select list (SELECT a + 1 AS x, {name}(x) OVER (...))")
        else:
            self.lit(")")
        self.ws()
        self.lit("OVER")
        self.ows()
        self.lit("(")
        self.ows()

        def partition() -> list[Col]:
            self.lit("PARTITION")
            self.ws()
            self.lit("BY")
            self.ws()
            cols = [self.column_name()]
            cols += self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), self.column_name())[3])
            return cols

        def sliding() -> tuple[int, int]:
            """ROWS BETWEEN (n PRECEDING | CURRENT ROW) AND (m FOLLOWING | CURRENT ROW) -> (n, m): both ends finite, BETWEEN
            mandatory"""
            def end(side: str) -> int:
                has_current, _ = self.attempt(lambda: (self.lit("CURRENT"), self.ws(), self.lit("ROW")))
                if has_current:
                    return 0
                digits = self.rx(_DIGITS)
                self.ws()
                self.lit(side)
                return int(digits)

            self.lit("ROWS")
            self.ws()
            self.lit("BETWEEN")
            self.ws()
            n = end("PRECEDING")
            self.ws()
            self.lit("AND")
            self.ws()
            return n, end("FOLLOWING")

        def frame() -> Any:
            """ROWS | RANGE  [BETWEEN]  UNBOUNDED PRECEDING  [AND CURRENT ROW] -> the unit, or the sliding frame -> what
            ``over(rows=)`` takes for it, (n, m): the only frames there are"""
            has_sliding, between = self.attempt(sliding)
            if has_sliding:
                return between
            unit = self.first_of(lambda: self.lit("ROWS"), lambda: self.lit("RANGE"))
            self.ws()
            self.attempt(lambda: (self.lit("BETWEEN"), self.ws()))
            self.lit("UNBOUNDED")
            self.ws()
            self.lit("PRECEDING")
            self.attempt(lambda: (self.ws(), self.lit("AND"), self.ws(), self.lit("CURRENT"), self.ws(), self.lit("ROW")))
            return unit

        has_partition, part = self.attempt(partition)
        if has_partition:
            has_order, order = self.attempt(lambda: (self.ws(), self.order_by_clause())[1])
        else:
            has_order, order = self.attempt(self.order_by_clause)
        if has_partition or has_order:
            has_frame, unit = self.attempt(lambda: (self.ws(), frame())[1])
        else:
            has_frame, unit = self.attempt(frame)
        self.ows()
        self.lit(")")
        keys = dict(partition_by=part if has_partition else [], order_by=order if has_order else [])
        rows: Any = has_frame and unit == "ROWS"  # what over(rows=) takes: True, False or the sliding frame's (n, m)
        if has_frame and type(unit) is tuple:
            rows, unit = unit, "ROWS BETWEEN"
        if ranking:
            if has_frame:
                raise ValueError(f"{name}() takes no frame clause ({unit} ...): a rank is a property of the row's place in its "
                                 "partition, not of a frame")
            item = WindowItem(name.lower()).over(**keys)
        elif name in _NAVIGATION:
            if name in ("LAG", "LEAD"):
                if len(extra) > 2:
                    raise ValueError(f"{name}({arg}, k, default) takes a column and two literals, not {len(extra)} behind it")
                item = WindowItem(name.lower(), arg, *extra)  # fewer than two: "k and the default are mandatory"
            elif name == "NTILE":
                item = F.ntile(extra[0])
            else:
                item = WindowItem(name.lower(), arg)
            if has_frame and name in ("LAG", "LEAD", "NTILE"):
                raise ValueError(f"{name}() takes no frame clause ({unit} ...): it is a property of the row's place in its "
                                 "partition, not of a frame")
            item = item.over(**keys, rows=rows)
        else:
            agg = F.count() if name == "COUNT" else {"SUM": F.sum, "AVG": F.avg, "MIN": F.min, "MAX": F.max}[name](arg)
            # RANGE is the default frame: through the last peer, which without ORDER BY is the whole partition
            item = agg.over(**keys, rows=rows)
        has_alias, alias = self.attempt(self.alias)
        self.saw_window_item = True
        return item.alias(alias) if has_alias else item

    def qualify_clause(self) -> Col:
        self.lit("QUALIFY")
        self.ws()
        return self.condition()

    def select_item(self) -> Col:
        return self.first_of(self.star, self.aggregate_call, self.expr_aliased)

    def star(self) -> Col:
        self.lit("*")
        return Col("*")

    def aggregate_call(self) -> AggCol:
        # ordered choice: the five aggregates as they were first, so COUNT(DISTINCT) - a column called DISTINCT - still
        # raises what it raised; COUNT(DISTINCT expr) did not parse at all before
        return self.first_of(self.plain_aggregate_call, self.count_distinct_call)

    def count_distinct_call(self) -> AggCol:
        self.lit("COUNT(DISTINCT")
        self.ws()
        arg = self.expr()
        self.lit(")")
        agg = F.count_distinct(_as_col(arg))
        has_alias, alias = self.attempt(self.alias)
        return agg.alias(alias) if has_alias else agg

    def plain_aggregate_call(self) -> AggCol:
        name = self.first_of(*[(lambda n=n: self.lit(n)) for n in _AGGREGATES])
        self.lit("(")
        has_arg, arg = self.attempt(self.expr)
        self.lit(")")
        has_alias, alias = self.attempt(self.alias)
        if name == "COUNT":
            if has_arg:
                raise AssertionError("COUNT takes no argument")
            agg = F.count()
        else:
            if not has_arg:
                raise AssertionError(f"{name} takes one argument")
            agg = {"SUM": F.sum, "AVG": F.avg, "MIN": F.min, "MAX": F.max}[name](_as_col(arg))
        return agg.alias(alias) if has_alias else agg

    def expr_aliased(self) -> Col:
        col = self.expr()
        has_alias, alias = self.attempt(self.alias)
        return _as_col(col).alias(alias) if has_alias else col

    def alias(self) -> str:
        self.ws()
        self.lit("AS")
        self.ws()
        return self.rx(_IDENT)

    def table_reference(self) -> DataFrame:
        self.lit("'")
        path = self.rx(_TABLE)
        self.lit("'")
        df = DataFrame(self.engine).table(path)
        has_alias, alias = self.attempt(self.alias)
        return df.alias(alias) if has_alias else df

    def join_clause(self) -> tuple[DataFrame, Col, str]:
        """-> (right table, condition, kind): "inner" for the reference's five spellings (it runs them all as the inner
        join), "left_semi" / "left_anti" for [LEFT] SEMI JOIN / [LEFT] ANTI JOIN, which are tried after those five."""
        def kind(words: tuple[str, ...], how: str) -> Callable[[], str]:
            def rule() -> str:
                self.lit(words[0])
                for w in words[1:]:
                    self.ws()
                    self.lit(w)
                return how
            return rule

        how = self.first_of(*[kind(words, "inner") for words in _JOIN_KINDS],
                            *[kind(words, how) for words, how in _SEMI_JOIN_KINDS])
        self.ws()
        table = self.table_reference()
        self.ws()
        self.lit("ON")
        self.ws()
        return table, self.condition(), how

    def where_clause(self) -> Col:
        self.lit("WHERE")
        self.ws()
        return self.condition()

    def group_by_clause(self) -> tuple[list[Col], Col | None, bool]:
        self.lit("GROUP")
        self.ws()
        self.lit("BY")
        self.ws()

        def bare() -> list[Col]:
            cols = [self.column_name()]
            cols += self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), self.column_name())[3])
            return cols

        def row() -> list[Col]:
            self.lit("(")
            self.ows()
            cols = bare()
            self.ows()
            self.lit(")")
            return cols

        # ordered choice: the bare form first (a column name never starts with a parenthesis), then the row form
        row_form, cols = False, None
        matched, cols = self.attempt(bare)
        if not matched:
            row_form, cols = True, row()

        def having() -> Col:
            self.ws()
            self.lit("HAVING")
            self.ws()
            return self.condition()

        has_having, cond = self.attempt(having)
        return cols, cond if has_having else None, row_form

    def order_by_clause(self) -> list[SortKey]:
        self.lit("ORDER")
        self.ws()
        self.lit("BY")
        self.ws()

        def key() -> SortKey:
            col = self.column_name()
            has_direction, word = self.attempt(lambda: (self.ws(), self.first_of(lambda: self.lit("ASC"),
                                                                                 lambda: self.lit("DESC")))[1])
            return col.desc() if has_direction and word == "DESC" else col.asc()

        keys = [key()]
        keys += self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), key())[3])
        return keys

    def limit_clause(self) -> int:
        self.lit("LIMIT")
        self.ws()
        return int(self.rx(_DIGITS))

    # ---- conditions -------------------------------------------------------------------------------------------
    def condition(self) -> Col:
        return self.or_expr()

    def or_expr(self) -> Col:
        left = self.and_expr()
        for right in self.repeat(lambda: (self.ws(), self.lit("OR"), self.ws(), self.and_expr())[3]):
            left = left | right
        return left

    def and_expr(self) -> Col:
        left = self.not_expr()
        for right in self.repeat(lambda: (self.ws(), self.lit("AND"), self.ws(), self.not_expr())[3]):
            left = left & right
        return left

    def not_expr(self) -> Col:
        negated, _ = self.attempt(lambda: (self.lit("NOT"), self.ws()))
        pred = self.predicate()
        return ~pred if negated else pred

    def predicate(self) -> Any:
        return self.first_of(self.comparison, self.parenthised_condition, self.string_literal, self.between, self.like)

    def comparison(self) -> Col:
        left = self.expr()
        self.ows()
        fn = self.first_of(*[(lambda s=s, f=f: (self.lit(s), f)[1]) for s, f in _COMPARATORS])
        self.ows()
        right = self.expr()
        return fn(left, right)

    def parenthised_condition(self) -> Col:
        self.lit("(")
        self.ows()
        cond = self.condition()
        self.ows()
        self.lit(")")
        return cond

    def between(self) -> Col:
        col = self.column_name()
        self.ws()
        self.lit("BETWEEN")
        self.ws()
        start = self.first_of(self.string_literal, self.column_name)
        self.ws()
        self.lit("AND")
        self.ws()
        end = self.first_of(self.string_literal, self.column_name)
        return col.between(start, end)

    def like(self) -> Col:
        col = self.expr()
        self.ws()
        self.lit("LIKE")
        self.ws()
        return _as_col(col).like(self.string_literal())

    # ---- arithmetic ---------------------------------------------------------------------------------------------
    def expr(self) -> Any:
        return self.add_expr()

    def _binary_chain(self, operand: Callable[[], Any], ops: dict[str, Callable[[Any, Any], Any]]) -> Any:
        left = operand()

        def tail() -> tuple[Callable[[Any, Any], Any], Any]:
            self.ows()
            fn = self.first_of(*[(lambda s=s, f=f: (self.lit(s), f)[1]) for s, f in ops.items()])
            self.ows()
            return fn, operand()

        for fn, right in self.repeat(tail):
            left = fn(left, right)
        return left

    def add_expr(self) -> Any:
        return self._binary_chain(self.mul_expr, {"+": operator.add, "-": operator.sub})

    def mul_expr(self) -> Any:
        return self._binary_chain(self.atom, {"*": operator.mul, "/": operator.truediv})

    def atom(self) -> Any:
        return self.first_of(self.function_call, self.number, self.case_expr, self.column_name, self.parenthised_expr,
                             self.string_literal)

    def case_expr(self) -> Col:
        """CASE WHEN cond THEN expr {WHEN cond THEN expr} ELSE expr END.  Tried before column_name: no text accepted
        without it holds a column followed by whitespace and WHEN, so a column called CASE still parses as a column."""
        def arm() -> tuple[Col, Any]:
            self.ws()
            self.lit("WHEN")
            self.ws()
            cond = self.condition()
            self.ws()
            self.lit("THEN")
            self.ws()
            return cond, self.expr()

        self.lit("CASE")
        arms = [arm()]
        arms += self.repeat(arm)
        self.ws()
        self.lit("ELSE")
        self.ws()
        col = _as_col(self.expr())
        self.ws()
        self.lit("END")
        if _IDENT_CHAR.match(self.text, self.pos):  # ENDFROM is no END; the other keywords are followed by whitespace
            self.fail()
        for cond, then in reversed(arms):
            col = CaseColumn(cond, _as_col(then), col)
        return col

    def function_call(self) -> Col:
        # COUNT(DISTINCT expr) after every form there was (HAVING COUNT(DISTINCT x) > 1, arithmetic over it)
        return self.first_of(self.plain_function_call, self.count_distinct_function)

    def count_distinct_function(self) -> Col:
        self.lit("COUNT")
        self.ows()
        self.lit("(")
        self.ows()
        self.lit("DISTINCT")
        self.ws()
        arg = self.expr()
        self.ows()
        self.lit(")")
        return F.count_distinct(_as_col(arg))

    def plain_function_call(self) -> Col:
        name = self.rx(_IDENT)
        self.ows()
        self.lit("(")
        self.ows()

        def arguments() -> list[Any]:
            args = [self.expr()]
            args += self.repeat(lambda: (self.ows(), self.lit(","), self.ows(), self.expr())[3])
            return args

        has_args, args = self.attempt(arguments)
        self.ows()
        self.lit(")")
        args = args if has_args else []
        if name == "COUNT":
            if args:
                raise AssertionError("COUNT takes no argument")
            return F.count()
        if name == "SUM":
            if len(args) != 1:
                raise AssertionError("SUM takes one argument")
            return F.sum(_as_col(args[0]))
        if name.lower() in DATE_PARTS and name.isupper():
            if len(args) != 1:
                raise AssertionError(f"{name} takes one argument")
            return DatePartColumn(name.lower(), _as_col(args[0]))
        if name == "DATE_TRUNC":
            if len(args) != 2:
                raise AssertionError("DATE_TRUNC takes a unit and one argument")
            return DateTruncColumn(args[0], _as_col(args[1]))  # the unit: a string literal, else ValueError
        raise SemanticError(f"Unsupported function: {name}")

    def parenthised_expr(self) -> Any:
        self.lit("(")
        self.ows()
        inner = self.expr()
        self.ows()
        self.lit(")")
        return inner

    # ---- terminals ----------------------------------------------------------------------------------------------
    def column_name(self) -> Col:
        return Col(self.rx(_COLUMN))

    def number(self) -> Lit:
        return Lit(int(self.rx(_NUMBER)))  # "1.5" -> ValueError, as in the reference (parser.py:349)

    def string_literal(self) -> str:
        self.lit("'")
        m = _STRING.match(self.text, self.pos)
        self.pos = m.end()
        self.lit("'")
        return m.group(0)


def _as_col(value: Any) -> Col:
    """A bare string literal used where a column expression is needed (e.g. SUM('x')) becomes a literal."""
    return value if isinstance(value, Col) else Lit(value)


def parse_sql(sql: str, engine: Any = None) -> DataFrame:
    """-> DataFrame bound to ``engine`` (None: the HIP engine is created on first use)."""
    parser = _Parser(sql, engine)
    try:
        return parser.query()
    except _NoMatch:
        at = parser.furthest
        raise SqlSyntaxError(f"not a supported query: cannot continue at offset {at}: {sql[at: at + 30]!r}") from None
