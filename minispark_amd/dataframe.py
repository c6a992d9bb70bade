"""Query builder with the reference's public surface (API to match: src/mini_spark/dataframe.py:28-86).

A ``DataFrame`` is a cursor over a growing chain of :mod:`minispark_amd.tasks` nodes; every builder call wraps the
current chain in one more node and hands the same object back, so calls chain.  What each call appends is declared
in ``_APPENDERS`` (method name -> node class + how the call's arguments map to the node's fields) and the methods
are generated from that table; only the calls that do more than append (``alias``, ``join``, running the query)
are written out.  Without an explicit engine the frame binds to the HIP engine on first use - this package has no
interpreted CPU engine.
"""

from __future__ import annotations

import copy
from pathlib import Path
from typing import Any, Callable

from . import tasks as _t
from .plan import PhysicalPlan
from .sql import KeyTupleCol, SortKey

# builder call -> (task class, arguments -> keyword fields of that class)
_APPENDERS: dict[str, tuple[type, Callable[..., dict[str, Any]]]] = {
    "table": (_t.LoadTableBlockTask, lambda file_path: {"file_path": Path(file_path)}),
    "select": (_t.ProjectTask, lambda *columns: {"columns": list(columns)}),
    "filter": (_t.FilterTask, lambda column: {"condition": column}),
}


class GroupedData:
    """``df.group_by(col)`` / ``df.group_by(col, col, ...)``: waits for ``agg(...)`` to become an aggregate node over ``df``'s chain."""

    def __init__(self, df: "DataFrame", column: Any) -> None:
        self.df, self.group_column = df, column

    def agg(self, *agg_columns: Any) -> "DataFrame":
        return self.df._append(_t.AggregateTask, group_by_column=self.group_column, agg_columns=list(agg_columns))


class DataFrame:
    def __init__(self, engine: Any = None) -> None:
        self._engine = engine
        self.task: _t.Task = _t.VoidTask()

    # ---- chain construction ------------------------------------------------------------------------------
    def _append(self, node_class: type, **fields: Any) -> "DataFrame":
        self.task = node_class(self.task, **fields)
        return self

    def alias(self, alias_name: str) -> "DataFrame":
        if type(self.task) is not _t.LoadTableBlockTask:
            raise AssertionError("Alias can only be applied to table")
        self.task.alias = alias_name
        return self

    def group_by(self, *columns: Any) -> GroupedData:
        """GROUP BY one column, or a tuple of up to eight plain columns of the input: the result then
        holds the key columns under their own names and types, in the order given, then the aggregates."""
        if not columns:
            raise TypeError("group_by() needs at least one column")
        if len(columns) == 1:
            return GroupedData(self, columns[0])
        if len(columns) > KeyTupleCol.MAX_PARTS:
            raise ValueError(f"GROUP BY takes at most {KeyTupleCol.MAX_PARTS} columns, not {len(columns)}")
        for col in columns:
            if type(col).__name__ not in {"Col", "SchemaCol"}:
                raise ValueError(f"GROUP BY over several columns takes plain columns, not the expression {col}: "
                                 "select(... .alias()) first")
        names = [col.name for col in columns]
        repeated = sorted({name for name in names if names.count(name) > 1})
        if repeated:
            raise ValueError(f"GROUP BY names a column twice: {repeated}")
        return GroupedData(self, KeyTupleCol(columns))

    def agg(self, *agg_columns: Any) -> "DataFrame":
        """Aggregates over the whole input, without GROUP BY: one row holding the aggregate columns in the order given,
        or no row when no input row is left (the value of grouping by a column that is equal in every row)."""
        if not agg_columns:
            raise ValueError("agg() needs at least one aggregate column")
        return self._append(_t.AggregateTask, group_by_column=None, agg_columns=list(agg_columns))

    def join(self, other_df: "DataFrame", on: Any, how: _t.JoinType) -> "DataFrame":
        """``how`` = "left_semi" / "left_anti": the rows of this frame with (without) a partner in ``other_df`` - this
        frame's columns, rows and order; ``on`` is one equality between a column of each side, optionally
        AND-ed with conditions over ``other_df``'s columns.  Every other kind runs as the inner join, as in the reference."""
        if how in ("left_semi", "left_anti"):
            return self._append(_t.SemiJoinTask, right_side_task=other_df.task, join_condition=on, anti=how == "left_anti")
        return self._append(_t.BroadcastHashJoinTask, right_side_task=other_df.task, join_condition=on, how=how)

    def order_by(self, *keys: Any) -> "DataFrame":
        """ORDER BY: ``Col`` (ascending), ``Col.asc()`` or ``Col.desc()``, the first key the most significant."""
        pairs = [(k.column, k.ascending) if isinstance(k, SortKey) else (k, True) for k in keys]
        top = self.task
        if type(top) is _t.SortTask and (top.distinct or top.windows) and not top.keys and top.limit is None:
            _t.check_sort_keys(pairs)  # directly above distinct() / window(): one task carries both, as limit() does
            top.keys = pairs
            return self
        if type(top) is _t.SortTask and top.distinct:
            raise ValueError("order_by() comes directly after distinct(), once, and before limit()")
        if type(top) is _t.SortTask and top.windows:
            raise ValueError("order_by() comes after window() / qualify() / distinct(), once, and before limit()")
        return self._append(_t.SortTask, keys=pairs)

    def window(self, *items: Any, select_order: list[str] | None = None) -> "DataFrame":
        """Window items over the result rows: every item - ``F.row_number()``, ``F.rank()`` or
        ``F.dense_rank()`` with ``.over(partition_by=[...], order_by=[...])``, or an aggregate ``F.sum(c)``, ``F.avg(c)``,
        ``F.min(c)``, ``F.max(c)``, ``F.count()`` with ``.over(partition_by=[...], order_by=[...], rows=False)``, or a
        navigation item ``F.lag(c, k, default)``, ``F.lead(c, k, default)``, ``F.first_value(c)``, ``F.last_value(c)``,
        ``F.ntile(n)`` with ``.over(...)``, and an optional ``.alias(name)`` - adds one column behind the existing ones
        (INTEGER for ranks, counts and NTILE, the argument's type for SUM / MIN / MAX and the value functions, FLOAT for
        AVG), in the order given; no row moves.  ``select_order`` (the SQL front end)
        names all columns in the order wanted instead.  It comes before ``qualify`` / ``distinct`` / ``order_by`` /
        ``limit``, which may name the new columns."""
        if not items:
            raise ValueError("window() needs at least one window item")
        top = self.task
        if type(top) is _t.SortTask:
            raise ValueError("window() comes once, before qualify() / distinct() / order_by() / limit()")
        return self._append(_t.SortTask, keys=[], limit=None, windows=list(items), select_order=select_order)

    def qualify(self, condition: Any) -> "DataFrame":
        """QUALIFY: a condition over the result's columns, the window columns among them, applied right after the
        windows were computed.  It follows ``window`` directly."""
        top = self.task
        if type(top) is not _t.SortTask or not top.windows:
            raise ValueError("qualify() follows window(): it filters on window columns")
        if top.qualify is not None or top.distinct or top.keys or top.limit is not None:
            raise ValueError("qualify() comes directly after window(), once, before distinct() / order_by() / limit()")
        top.qualify = condition
        return self

    def distinct(self) -> "DataFrame":
        """SELECT DISTINCT: of the rows that are equal in every column the first stays.  It comes before ``order_by`` /
        ``limit``, which then apply to the rows that are left."""
        top = self.task
        if type(top) is _t.SortTask and top.windows and not top.distinct and not top.keys and top.limit is None:
            top.distinct = True  # above window() / qualify(): one task carries all of them
            return self
        if type(self.task) is _t.SortTask:
            raise ValueError("distinct() was already applied" if self.task.distinct and not self.task.keys
                             and self.task.limit is None else "distinct() comes before order_by() / limit()")
        return self._append(_t.SortTask, keys=[], limit=None, distinct=True)

    def limit(self, n: int) -> "DataFrame":
        """LIMIT: of an ``order_by`` directly below, else the first ``n`` rows in the engine's own order."""
        _t.check_limit(n)
        if type(self.task) is _t.SortTask:
            self.task.limit = n
            return self
        return self._append(_t.SortTask, keys=[], limit=n)

    # ---- binding + execution ---------------------------------------------------------------------------------
    @property
    def engine(self) -> Any:
        if self._engine is None:
            from .execution import HipExecutionEngine  # noqa: PLC0415 - loads libhipspark.so, needs a GPU

            self._engine = HipExecutionEngine()
        return self._engine

    @engine.setter
    def engine(self, engine: Any) -> None:
        self._engine = engine

    @property
    def schema(self) -> Any:
        return self.task.validate_schema()

    def _rows(self, limit: float | None = None) -> list:
        engine = self.engine
        results = engine.execute_full_task(self.task)
        rows = engine.collect_results(results) if limit is None else engine.collect_results(results, limit=limit)
        return list(rows)

    def collect(self) -> list:
        return self._rows()

    def collect_columns(self) -> dict:
        """The result column-wise: name -> numpy array (or list of str) - see ExecutionEngine.collect_columns."""
        engine = self.engine
        return engine.collect_columns(engine.execute_full_task(self.task))

    def show(self, n: int = 10) -> int:
        import tabulate  # noqa: PLC0415

        rows = self._rows(limit=n)
        print(tabulate.tabulate(rows, headers="keys", tablefmt="rounded_outline"))  # noqa: T201
        return len(rows)

    def explain(self, *, full: bool = False) -> None:
        snapshot = copy.deepcopy(self.task)  # planning annotates the nodes it is given
        print("Logical Plan")  # noqa: T201
        snapshot.explain()
        if full:
            PhysicalPlan.generate_physical_plan(snapshot).explain()


def _make_appender(name: str, node_class: type, to_fields: Callable[..., dict[str, Any]]) -> Callable[..., DataFrame]:
    def method(self: DataFrame, *args: Any, **kwargs: Any) -> DataFrame:
        return self._append(node_class, **to_fields(*args, **kwargs))

    method.__name__ = method.__qualname__ = name
    method.__doc__ = f"Wrap the chain in a {node_class.__name__}."
    return method


for _name, (_cls, _to_fields) in _APPENDERS.items():
    setattr(DataFrame, _name, _make_appender(_name, _cls, _to_fields))
