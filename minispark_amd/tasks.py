"""Logical / physical operator nodes of a query (reference: src/mini_spark/tasks.py).

Host-side mirror of the reference's ``Task`` classes: same class names, same fields, same schema
rules and error messages - so a plan built by the reference lowers through the same code as one built
here (:mod:`minispark_amd.lowering` dispatches on class names).  Unlike the reference the nodes carry
**no row-processing code**: the reference's ``generate_chunks`` / ``execute`` / ``write`` bodies
(tasks.py:117-121,167-177,201-240,270-310,347-375,400-410) are what the HIP kernels replace.

Nodes form a linked list through ``parent_task`` (a join also has ``right_side_task``); ``VoidTask``
terminates the list.
"""

from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterator, Literal

from .constants import ColumnType, Schema
from .io import BlockFile
from .sql import BINOP_SYMBOLS, AggCol, BinaryOperatorColumn, Col, KeyTupleCol, LikeColumn

JoinType = Literal["inner", "left", "right", "outer", "left_semi", "left_anti"]


def nice_schema(schema: Schema | None) -> str:
    if schema is None:
        return ""
    return "[" + ", ".join(f"{name}:{col_type}" for name, col_type in schema) + "]"


def _plain_column_names(*exprs: Col) -> list[str]:
    return [c.name for e in exprs for c in e.all_nested_columns if type(c).__name__ == "Col"]


def _check_known(exprs: list[Col], schema: Schema, where: str) -> None:
    known = {name for name, _ in schema}
    unknown = [n for n in dict.fromkeys(_plain_column_names(*exprs)) if n not in known]
    if unknown:
        raise ValueError(f"Unknown columns in {where}: {unknown}")


@dataclass
class Task:
    parent_task: "Task" = field(repr=False)
    inferred_schema: Schema | None = None

    def validate_schema(self) -> Schema:
        return self.parent_task.validate_schema()

    @property
    def task_chain(self) -> Iterator["Task"]:
        if type(self) is VoidTask:
            return
        yield from self.parent_task.task_chain
        yield self

    def describe(self) -> str:
        return type(self).__name__

    def explain(self, lvl: int = 0) -> None:
        indent = "  " * lvl + ("+- " if lvl > 0 else "")
        print(f"{indent} {self.describe()}:{nice_schema(self.inferred_schema)}")  # noqa: T201
        self.parent_task.explain(lvl + 1)


@dataclass
class VoidTask(Task):
    parent_task: Task | None = None  # type: ignore[assignment]

    def validate_schema(self) -> Schema:
        return []

    def explain(self, lvl: int = 0) -> None:
        pass


@dataclass(kw_only=True)
class ProducerTask(Task):
    pass


@dataclass(kw_only=True)
class ConsumerTask(Task):
    pass


@dataclass(kw_only=True)
class WriterTask(Task):
    pass


@dataclass(kw_only=True)
class LoadTableBlockTask(ProducerTask):
    """Scan of one BlockFile; one job per file block (tasks.py:112-138)."""

    file_path: Path
    alias: str = ""

    @property
    def file_schema(self) -> Schema:
        return BlockFile(self.file_path).file_schema

    def validate_schema(self) -> Schema:
        if self.parent_task.validate_schema() != []:
            raise AssertionError("a table scan has no input")
        if not self.alias:
            return list(self.file_schema)
        return [(f"{self.alias}.{name}", col_type) for name, col_type in self.file_schema]

    def describe(self) -> str:
        return f"LoadTableBlockTask({self.file_path})"


@dataclass(kw_only=True)
class LoadShuffleFilesTask(ProducerTask):
    """Reads back what the previous stage shuffled; one job per partition (tasks.py:141-156)."""

    def describe(self) -> str:
        return "LoadShuffleFile()"


@dataclass(kw_only=True)
class ProjectTask(ConsumerTask):
    columns: list[Col]

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        expanded: list[Col] = []
        for col in self.columns:
            if type(col).__name__ == "Col" and col.name == "*":
                expanded.extend(Col(name) for name, _ in schema)
            else:
                expanded.append(col)
        self.columns = expanded
        _check_known(self.columns, schema, "projection")
        return [(col.name, col.infer_type(schema)) for col in self.columns]

    def describe(self) -> str:
        return f"Project({', '.join(str(c) for c in self.columns)})"


@dataclass(kw_only=True)
class FilterTask(ConsumerTask):
    condition: Col

    def __post_init__(self) -> None:
        if type(self.condition).__name__ not in {"BinaryOperatorColumn", "LikeColumn"}:
            raise AssertionError(type(self.condition))

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        self.condition.infer_type(schema)
        return schema

    def describe(self) -> str:
        return f"Filter({self.condition})"


@dataclass(kw_only=True)
class BroadcastHashJoinTask(ProducerTask):
    """Inner equi-join on one column pair.  Despite the name both inputs are hash-partitioned on the
    key; the LEFT input (``parent_task``) is the build side (tasks.py:190-260)."""

    right_side_task: Task
    join_condition: Col
    how: JoinType = "inner"
    left_key: Col | None = None
    right_key: Col | None = None
    left_schema: Schema | None = None
    right_schema: Schema | None = None

    def validate_schema(self) -> Schema:
        self.left_schema = self.parent_task.validate_schema()
        self.right_schema = self.right_side_task.validate_schema()
        _check_known([self.join_condition], self.left_schema + self.right_schema, "Join")
        if type(self.join_condition).__name__ != "BinaryOperatorColumn":
            raise AssertionError("Only equi-join is supported")
        self.left_key, self.right_key = self.join_condition.extract_left_right_key(
            self.left_schema, self.right_schema
        )
        return self.left_schema + self.right_schema

    def describe(self) -> str:
        return f'Join({self.join_condition}, "{self.how}")'

    def explain(self, lvl: int = 0) -> None:
        indent = "  " * lvl + ("+- " if lvl > 0 else "")
        print(f"{indent} {self.describe()}:{nice_schema(self.inferred_schema)}")  # noqa: T201
        self.parent_task.explain(lvl + 1)
        self.right_side_task.explain(lvl + 1)


def _conjuncts(cond: Col) -> list[Col]:
    """The operands of the AND chain on top of a condition, left to right."""
    if type(cond).__name__ == "BinaryOperatorColumn" and BINOP_SYMBOLS[cond.operator] == "and":
        return [*_conjuncts(cond.left_side), *_conjuncts(cond.right_side)]
    return [cond]


SEMI_KEY_TYPES = (ColumnType.INTEGER, ColumnType.STRING, ColumnType.TIMESTAMP)


@dataclass(kw_only=True)
class SemiJoinTask(ProducerTask):
    """LEFT SEMI / LEFT ANTI join (no reference counterpart: DESIGN.md 4.4j): the rows of the LEFT input (``parent_task``)
    whose key occurs (``anti``: does not occur) in the right input's key column - the left input's columns, rows and order,
    i.e. ``left WHERE key IN {right keys}``.  ``join_condition`` is one equality between a plain column of each side,
    optionally AND-ed with conditions over right-side columns only (``... ON o_orderkey = l_orderkey AND l_commitdate <
    l_receiptdate``); ``validate_schema`` resolves it into ``left_key``, ``right_key`` and ``right_filters``, which the planner
    places on the right input.  A class of its own, not a ``how`` of the inner join: nothing that matches the inner join by
    name - fused probes, native stages - can take it for one."""

    right_side_task: Task
    join_condition: Col
    anti: bool = False
    left_key: Col | None = None
    right_key: Col | None = None
    right_filters: list[Col] = field(default_factory=list)
    left_schema: Schema | None = None
    right_schema: Schema | None = None
    expanded: bool = False  # the planner has moved right_filters below the right input's key projection

    @property
    def how(self) -> str:
        return "left_anti" if self.anti else "left_semi"

    def validate_schema(self) -> Schema:
        self.left_schema = self.parent_task.validate_schema()
        self.right_schema = self.right_side_task.validate_schema()
        if not self.expanded:
            self._resolve_condition()
        left_type = self.left_key.infer_type(self.left_schema)
        right_type = self.right_key.infer_type(self.right_schema)
        if left_type != right_type or left_type not in SEMI_KEY_TYPES:
            raise TypeError(f"{self.how} join on {self.left_key.name}:{left_type} = {self.right_key.name}:{right_type}: the keys "
                            "are two INTEGER, two STRING or two TIMESTAMP columns (a FLOAT key has no exact equality)")
        return list(self.left_schema)

    def _resolve_condition(self) -> None:
        left_names = {n for n, _ in self.left_schema}
        right_names = {n for n, _ in self.right_schema}
        _check_known([self.join_condition], self.left_schema + self.right_schema, "Join")
        key, filters = None, []
        for part in _conjuncts(self.join_condition):
            names = set(_plain_column_names(part))
            on_left, on_right = names & left_names, names & right_names
            if on_left & on_right:
                raise ValueError(f"{self.how} join: {part} names {sorted(on_left & on_right)}, which both inputs hold: alias() "
                                 "the tables")
            if on_left and on_right:
                is_key = (type(part).__name__ == "BinaryOperatorColumn" and BINOP_SYMBOLS[part.operator] == "=="
                          and type(part.left_side).__name__ == "Col" and type(part.right_side).__name__ == "Col")
                if not is_key or key is not None:
                    raise ValueError(f"{self.how} join: the condition {part} reads both inputs; beside ONE equality between a "
                                     "plain column of each side, a condition may read the right input only")
                key = part
            elif on_left:
                raise ValueError(f"{self.how} join: the condition {part} reads the left input only: it belongs in WHERE "
                                 "(filter() the left input)")
            else:
                if type(part).__name__ not in {"BinaryOperatorColumn", "LikeColumn"}:
                    raise ValueError(f"{self.how} join: {part} is no condition")
                part.infer_type(self.right_schema)
                filters.append(part)
        if key is None:
            raise ValueError(f"{self.how} join: the condition {self.join_condition} holds no equality between a plain column of "
                             "each side")
        self.left_key, self.right_key = key.extract_left_right_key(self.left_schema, self.right_schema)
        self.right_filters = filters

    def describe(self) -> str:
        return f'SemiJoin({self.join_condition}, "{self.how}")'

    def explain(self, lvl: int = 0) -> None:
        indent = "  " * lvl + ("+- " if lvl > 0 else "")
        print(f"{indent} {self.describe()}:{nice_schema(self.inferred_schema)}")  # noqa: T201
        self.parent_task.explain(lvl + 1)
        self.right_side_task.explain(lvl + 1)


@dataclass(kw_only=True)
class AggregateTask(ConsumerTask):
    """Hash group-by on ONE plain column.  ``before_shuffle`` = the per-job partial phase, otherwise
    the merge phase that combines column i+1 of the shuffled partial rows with aggregate i
    (tasks.py:263-340).  ``group_by_column=None`` (no reference counterpart) aggregates the whole input: the value of
    grouping by a column that is equal in every row, without that column - one row, or none when no row came in.
    A ``KeyTupleCol`` (no reference counterpart either) groups by several columns: the logical node yields the key columns
    under their own names and types, then the aggregates; in the physical plan the partial and the merging node see the
    tuple as one packed STRING column and an ``UnpackKeyTask`` above the merge restores the key columns."""

    group_by_column: Col | None
    agg_columns: list[AggCol]
    before_shuffle: bool = True

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        if not self.before_shuffle:
            return schema
        if self.group_by_column is None:
            _check_known(list(self.agg_columns), schema, "aggregation")
            return [(agg.name, agg.infer_type(schema)) for agg in self.agg_columns]
        _check_known([*self.agg_columns, self.group_by_column], schema, "aggregation")
        key = self.group_by_column
        key_schema = (key.part_schema(schema) if type(key) is KeyTupleCol and not key.packed
                      else [(key.name, key.infer_type(schema))])
        return [*key_schema, *[(agg.name, agg.infer_type(schema)) for agg in self.agg_columns]]

    def describe(self) -> str:
        if self.group_by_column is None:
            return f"AggregateTask(whole input, agg: {self.agg_columns}, before_shuffle:{self.before_shuffle})"
        return (
            f"AggregateTask(group_by: {self.group_by_column}, agg: {self.agg_columns}, "
            f"before_shuffle:{self.before_shuffle})"
        )


@dataclass(kw_only=True)
class UnpackKeyTask(ConsumerTask):
    """Directly above the merging aggregate of a GROUP BY over several columns (no reference counterpart): column 0, the
    packed key tuple, is cut back into the key columns ``part_schema`` names - their own names and types, in the order
    given - and the aggregates follow unchanged."""

    key: KeyTupleCol
    part_schema: Schema

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        if not schema or schema[0][0] != self.key.name:
            raise AssertionError(f"UnpackKeyTask expects the packed key {self.key.name} in column 0, got {schema}")
        return [*self.part_schema, *schema[1:]]

    def describe(self) -> str:
        return f"UnpackKey({self.key} <- {self.key.name})"


MARK_TYPES = (ColumnType.INTEGER, ColumnType.FLOAT, ColumnType.TIMESTAMP)


@dataclass(kw_only=True)
class MarkFirstTask(ConsumerTask):
    """Directly under the partial aggregate of a query with COUNT(DISTINCT e) (no reference counterpart: DESIGN.md 4.4e).
    For every item (reserved mark name, argument expression) the input gains one INTEGER column: 1 in a row that survives
    the WHERE and is the first such row, in input order, with its values of (the parts of ``key``, the argument), else 0 -
    so the partial aggregate's ``SUM(mark)`` per group is the number of different arguments.  ``key`` = the GROUP BY key
    of that aggregate: None (whole input), a plain column, or the ``KeyTupleCol`` in its unpacked form.  An argument is a
    plain column of any type or an INTEGER / FLOAT / TIMESTAMP valued expression, compared as the value ``select`` would
    store.  Refused here, at planning: a FLOAT key column (the aggregation tiers group floats by their own rule, and the
    marks must not disagree with them about -0.0 or NaN), a computed key, a string-valued or boolean argument expression."""

    key: Col | None
    items: list[tuple[str, Col]]

    def key_parts(self) -> list[Col]:
        if self.key is None:
            return []
        return list(self.key.parts) if type(self.key) is KeyTupleCol else [self.key]

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        for part in self.key_parts():
            if type(part).__name__ not in {"Col", "SchemaCol"}:
                raise NotImplementedError(f"COUNT(DISTINCT) under GROUP BY {part}: the key must be a plain column, not an "
                                          "expression: select(... .alias()) it first")
            if part.infer_type(schema) == ColumnType.FLOAT:
                raise NotImplementedError(f"COUNT(DISTINCT) under GROUP BY {part.name}: a FLOAT key column is not supported "
                                          "(group by an INTEGER, STRING or TIMESTAMP column instead)")
        _check_known([expr for _, expr in self.items], schema, "COUNT(DISTINCT)")
        for _, expr in self.items:
            bare = expr
            while type(bare).__name__ == "AliasColumn":
                bare = bare.original_col
            if type(bare).__name__ in {"Col", "SchemaCol"}:
                bare.infer_type(schema)
                continue
            boolean = (type(bare).__name__ == "LikeColumn" or
                       (type(bare).__name__ == "BinaryOperatorColumn" and
                        BINOP_SYMBOLS[bare.operator] in {"==", "!=", "<", "<=", ">", ">=", "and", "or"}))
            if boolean or bare.infer_type(schema) not in MARK_TYPES:
                raise NotImplementedError(f"COUNT(DISTINCT {expr}): the argument is a column or an INTEGER / FLOAT / TIMESTAMP "
                                          "valued expression; select(... .alias()) a string expression first and count the "
                                          "column")
        return [*schema, *[(name, ColumnType.INTEGER) for name, _ in self.items]]

    def describe(self) -> str:
        key = "whole input" if self.key is None else f"key: {self.key}"
        return f"MarkFirst({key}; " + ", ".join(f"{name} <- {expr}" for name, expr in self.items) + ")"


@dataclass(kw_only=True)
class SortTask(ConsumerTask):
    """ORDER BY / LIMIT over the query's result rows (no reference counterpart).  ``keys`` = (plain column of the input
    schema, ascending) pairs, the first the most significant; ``limit`` = rows kept (None: all).  Without keys the
    first ``limit`` rows are kept in the engine's own order.  Always the last logical operation: the engine runs it on
    the finished result, after the values were rounded to their stored types.  ``distinct`` (SELECT DISTINCT): rows
    equal in EVERY column are removed first - the first of them in the result's order stays - and keys and limit apply
    to the survivors.  It rides on this task so that every guard ORDER BY has holds for it unchanged."""

    keys: list[tuple[Col, bool]] = field(default_factory=list)
    limit: int | None = None
    distinct: bool = False
    # window items: ``windows`` = sql.WindowItem list, each one column added to the input's
    # columns; ``qualify`` = a condition over all of them (QUALIFY), applied right after; ``select_order`` = the names of
    # all output columns in the order wanted (None: the input's columns, then the windows).  They run BEFORE distinct,
    # keys and limit, which may name the window columns.
    windows: list = field(default_factory=list)
    qualify: Col | None = None
    select_order: list[str] | None = None

    MAX_WINDOWS = 8

    def __post_init__(self) -> None:
        check_sort_keys(self.keys)
        if self.limit is not None:
            check_limit(self.limit)
        check_windows(self.windows)

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        self.input_schema = list(schema)  # what the windows read: the engine finds their keys here by position
        if self.windows:
            check_windows(self.windows)
            for item in self.windows:
                for col in [*item.partition_by, *[c for c, _ in item.order_by]]:
                    col.infer_type(schema)  # a key is a column of the INPUT, never another window item
            # ... and so is an aggregate's argument; every item adds a column of its own type (INTEGER: ranking and COUNT)
            schema = [*schema, *[(item.name, item.out_type(self.input_schema)) for item in self.windows]]
            names = [name for name, _ in schema]
            repeated = sorted({name for name in names if names.count(name) > 1})
            if repeated:
                raise ValueError(f"Duplicate column names in window(): {repeated} (alias() the window item)")
            if self.select_order is not None:
                if sorted(self.select_order) != sorted(names):
                    raise ValueError(f"window(): the column order {self.select_order} does not name the columns {names}")
                types = dict(schema)
                schema = [(name, types[name]) for name in self.select_order]
        elif self.qualify is not None:
            raise ValueError("QUALIFY filters on window columns: the query has no window item")
        if self.qualify is not None:
            _check_known([self.qualify], schema, "QUALIFY")
        for col, _ in self.keys:
            col.infer_type(schema)  # ValueError('Column "x" not found in schema ...')
        return schema

    def __repr__(self) -> str:
        """The dataclass form; ``distinct`` and the window fields are named only when set, so a plain task prints as it
        did before they existed."""
        quiet = {"distinct", "windows", "qualify", "select_order"}
        shown = [f for f in dataclasses.fields(self) if f.repr and (f.name not in quiet or getattr(self, f.name))]
        return f"{type(self).__name__}(" + ", ".join(f"{f.name}={getattr(self, f.name)!r}" for f in shown) + ")"

    def describe(self) -> str:
        keys = ", ".join(f"{col} {'ASC' if ascending else 'DESC'}" for col, ascending in self.keys)
        plain = f"Sort({'DISTINCT ' if self.distinct else ''}{keys}; limit={self.limit})"
        if not self.windows and self.qualify is None:
            return plain
        qualify = "" if self.qualify is None else f"; QUALIFY {self.qualify}"
        return f"Window({'; '.join(str(item) for item in self.windows)}{qualify}) -> {plain}"


def check_windows(windows: list) -> None:
    if len(windows) > SortTask.MAX_WINDOWS:
        raise ValueError(f"a query takes at most {SortTask.MAX_WINDOWS} window items, not {len(windows)}")
    for item in windows:
        if type(item).__name__ != "WindowItem" or not item.is_over:
            raise ValueError("window() takes F.row_number() / F.rank() / F.dense_rank() or F.sum(c) / F.avg(c) / F.min(c) / "
                             f"F.max(c) / F.count() with .over(...), not {item}")
        if len(item.partition_by) + len(item.order_by) > MAX_WINDOW_KEYS:
            raise ValueError(f"{item}: partition and order columns together are at most {MAX_WINDOW_KEYS} (HS_MAX_COLS)")


MAX_WINDOW_KEYS = 12  # include/hipspark.h HS_MAX_COLS


def check_sort_keys(keys: list) -> None:
    for col, _ in keys:
        if type(col).__name__ not in {"Col", "SchemaCol"}:
            raise ValueError(f"ORDER BY takes plain columns, not the expression {col}: select(... .alias()) first")


def check_limit(n: object) -> None:
    if type(n) is not int or n < 0:
        raise ValueError(f"LIMIT takes an int >= 0, not {n!r}")


@dataclass
class WriteToShufflePartitions(WriterTask):
    """Stage boundary: rows are routed by ``hash(key) % SHUFFLE_PARTITIONS`` and quantised to the
    on-disk types (FLOAT->f32, INTEGER->i32) - tasks.py:343-397."""

    key_column: Col | None = None

    def validate_schema(self) -> Schema:
        schema = self.parent_task.validate_schema()
        if self.key_column is None:
            return schema
        known = {name for name, _ in schema}
        if type(self.key_column) is KeyTupleCol and self.key_column.name in known:
            return schema  # the packed key tuple: its parts stayed behind the partial aggregate
        unknown = [n for n in _plain_column_names(self.key_column) if n not in known]
        if unknown:
            raise ValueError(f"Unknown columns in GroupBy: {unknown}")
        if self.key_column.name in known:
            return schema
        return [(self.key_column.name, self.key_column.infer_type(schema)), *schema]

    def describe(self) -> str:
        return f"WriteToShufflePartitions({self.key_column})"


@dataclass(kw_only=True)
class WriteToLocalFileTask(WriterTask):
    def describe(self) -> str:
        return "WriteToLocalFileTask()"


__all__ = [
    "AggregateTask",
    "BinaryOperatorColumn",
    "BroadcastHashJoinTask",
    "ConsumerTask",
    "FilterTask",
    "JoinType",
    "LikeColumn",
    "LoadShuffleFilesTask",
    "LoadTableBlockTask",
    "MarkFirstTask",
    "ProducerTask",
    "ProjectTask",
    "SemiJoinTask",
    "SortTask",
    "Task",
    "UnpackKeyTask",
    "VoidTask",
    "WriteToLocalFileTask",
    "WriteToShufflePartitions",
    "WriterTask",
    "nice_schema",
]
