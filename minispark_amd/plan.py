"""Physical planning: logical task chain -> barrier-separated stages (reference: src/mini_spark/plan.py).

This is the build's own counterpart of the *caller* of the hot path: it decides
what the units of work are, and those units are part of the result semantics:

* one unit of partial aggregation per **file block** (``LoadTableBlockTask`` producer, plan.py:90-93);
* after a join, one unit per **shuffle partition** (``BroadcastHashJoinTask`` producer, plan.py:99-109);
* all partial rows of a key meet in exactly one final-merge unit (``LoadShuffleFilesTask``, plan.py:94-98).

Rewrites applied, in the reference's order (plan.py:224-235):

1. wrap the chain in ``WriteToLocalFileTask``; infer schemas bottom-up;
2. ``expand``: AggregateTask -> [Aggregate(before_shuffle) -> WriteToShufflePartitions(key) ->
   LoadShuffleFiles -> Aggregate(after)] (+ ProjectTask computing AVG = sum/count, plan.py:190-203); an aggregate
   without GROUP BY (this build's own) expands alike with ``key=None`` and no key column in the projection;
   join inputs each get a WriteToShufflePartitions on their key (plan.py:186-189);
   2a. a GROUP BY over several columns (``KeyTupleCol``, this build's own): both aggregates and the shuffle write see the
   tuple as ONE packed STRING column under the tuple's reserved name, and an ``UnpackKeyTask`` directly above the merging
   aggregate - below the AVG projection, HAVING, the final select and any ``SortTask`` - restores the key columns;
   2c. a ``SemiJoinTask`` (LEFT SEMI / LEFT ANTI join, this build's own): the right input becomes
   right -> Filter(each right-side conjunct of the condition) -> Project(right key), so only the key column is
   materialised; both inputs get a WriteToShufflePartitions on their key as a join's do, and the stage is cut there;
   2b. ``COUNT(DISTINCT e)`` (this build's own): one ``MarkFirstTask`` directly under the partial aggregate
   appends a first-occurrence mark column per distinct argument, and the aggregate carries ``SUM(mark)`` under the
   requested name in its place (the ``expand_avg`` pattern) - the merge and everything above it see an integer SUM;
3. strip ``alias.`` prefixes from the output column names with a final ProjectTask (plan.py:207-222);
4. cut the chain into stages at every shuffle write / join, dependencies first.

A ``SortTask`` (ORDER BY / LIMIT, this build's own) must top the chain; it ends up among the consumers of the stage that
writes the result, below rewrite 3's rename-only ProjectTask, and the engine runs it on the finished rows.
"""

from __future__ import annotations

from copy import deepcopy

from .sql import AggCol, Col, KeyTupleCol
from .tasks import (
    AggregateTask,
    BroadcastHashJoinTask,
    ConsumerTask,
    FilterTask,
    LoadShuffleFilesTask,
    MarkFirstTask,
    ProducerTask,
    ProjectTask,
    SemiJoinTask,
    SortTask,
    Task,
    UnpackKeyTask,
    VoidTask,
    WriterTask,
    WriteToLocalFileTask,
    WriteToShufflePartitions,
)


class Stage:
    """producer -> consumers -> writer; ``dependencies`` are the stages whose shuffle output it reads
    (for a join: [left/build stage, right/probe stage])."""

    def __init__(self, full_task: Task, dependencies: list["Stage"]) -> None:
        self.full_task = full_task
        self.dependencies = dependencies
        self.stage_id = ""
        self.job_results: list = []
        chain = list(full_task.task_chain)
        producer, consumers, writer = chain[0], chain[1:-1], chain[-1]
        if not isinstance(producer, ProducerTask):
            raise AssertionError(f"stage must start with a producer, got {type(producer).__name__}")
        if not all(isinstance(c, ConsumerTask) for c in consumers):
            raise AssertionError("stage interior must be consumers")
        if not isinstance(writer, WriterTask):
            raise AssertionError(f"stage must end with a writer, got {type(writer).__name__}")
        self.producer: ProducerTask = producer
        self.consumers: list[ConsumerTask] = consumers  # type: ignore[assignment]
        self.writer: WriterTask = writer

    def late_initialize(self, stage_id: str) -> None:
        self.stage_id = stage_id

    def explain(self) -> None:
        self.full_task.explain()

    def __repr__(self) -> str:
        consumers = f"[{','.join(type(c).__name__ for c in self.consumers)}] -> " if self.consumers else ""
        deps = ",".join(str(d.stage_id) for d in self.dependencies)
        return (
            f"[Stage {self.stage_id}: {type(self.producer).__name__} -> {consumers}"
            f"{type(self.writer).__name__}, deps: ({deps})]"
        )


def _cut(top: Task) -> Stage:
    """Detach ``top``'s chain at the first shuffle boundary below it and build stages recursively.

    ``top`` is always a writer.  Walking down from it, the stage ends either at a join (whose two
    inputs are separate stages) or where the parent is a WriteToShufflePartitions (which tops the
    next stage down)."""
    node = top
    while True:
        if type(node) in (BroadcastHashJoinTask, SemiJoinTask):
            left_top, right_top = node.parent_task, node.right_side_task
            node.parent_task, node.right_side_task = VoidTask(), VoidTask()
            return Stage(top, [_cut(left_top), _cut(right_top)])
        parent = node.parent_task
        if parent is None or type(parent) is VoidTask:
            return Stage(top, [])
        if type(parent) is WriteToShufflePartitions:
            node.parent_task = VoidTask()
            return Stage(top, [_cut(parent)])
        node = parent


def _execution_order(stage: Stage, out: list[Stage]) -> None:
    for dep in stage.dependencies:
        _execution_order(dep, out)
    out.append(stage)


class PhysicalPlan:
    def __init__(self, stages: list[Stage]) -> None:
        self.stages = stages

    @staticmethod
    def infer_schema(task: Task) -> None:
        node: Task | None = task
        while node is not None and type(node) is not VoidTask:
            node.inferred_schema = node.validate_schema()
            if type(node) in (BroadcastHashJoinTask, SemiJoinTask):
                PhysicalPlan.infer_schema(node.right_side_task)
            node = node.parent_task

    @staticmethod
    def expand_tasks(task: Task) -> Task:
        if type(task) is VoidTask:
            return task
        task.parent_task = PhysicalPlan.expand_tasks(task.parent_task)
        if type(task) is BroadcastHashJoinTask:
            task.right_side_task = PhysicalPlan.expand_tasks(task.right_side_task)
            task.parent_task = WriteToShufflePartitions(task.parent_task, key_column=task.left_key)
            task.right_side_task = WriteToShufflePartitions(task.right_side_task, key_column=task.right_key)
            return task
        if type(task) is SemiJoinTask:
            # the right input is a key SET: its conditions, then the key column alone (rewrite 2c); both inputs end in a
            # shuffle write as a join's do - no row moves here, the write quantises them to their stored types
            right = PhysicalPlan.expand_tasks(task.right_side_task)
            for cond in task.right_filters:
                right = FilterTask(right, condition=cond)
            right = ProjectTask(right, columns=[Col(task.right_key.name)])
            task.parent_task = WriteToShufflePartitions(task.parent_task, key_column=task.left_key)
            task.right_side_task = WriteToShufflePartitions(right, key_column=task.right_key)
            task.expanded = True
            return task
        if type(task) is AggregateTask and task.before_shuffle:
            requested = task.agg_columns
            # COUNT(DISTINCT e) is carried as SUM(mark) (rewrite 2b); counts of one argument share a mark column
            marks: dict[str, tuple[str, Col]] = {}
            carried = []
            for agg in requested:
                if agg.type != "count_distinct":
                    carried.extend(agg.expand_avg())
                    continue
                arg = agg.original_col
                name, _ = marks.setdefault(str(arg), (f"__hs_mark{len(marks)}({arg.name})", arg))
                carried.append(AggCol("sum", Col(name)).alias(agg.name))
            below = task.parent_task
            if marks:
                below = MarkFirstTask(below, key=task.group_by_column, items=list(marks.values()))
            key_tuple = task.group_by_column if type(task.group_by_column) is KeyTupleCol else None
            if key_tuple is not None:
                # several key columns: from the partial aggregate to the merge they are ONE packed column (rewrite 2a)
                part_schema = list(task.inferred_schema[: len(key_tuple.parts)])
                task.group_by_column = key_tuple.as_packed()
            partial = AggregateTask(below, group_by_column=task.group_by_column, agg_columns=carried)
            shuffled = WriteToShufflePartitions(partial, key_column=task.group_by_column)
            task.parent_task = LoadShuffleFilesTask(shuffled)
            task.before_shuffle = False
            task.agg_columns = [AggCol(agg.type, Col(agg.name)) for agg in carried]
            top: Task = task
            if key_tuple is not None:
                top = UnpackKeyTask(task, key=task.group_by_column, part_schema=part_schema)
            if any(agg.type == "avg" for agg in requested):
                if key_tuple is not None:
                    key = [Col(part.name) for part in key_tuple.parts]
                else:
                    key = [] if task.group_by_column is None else [Col(task.group_by_column.name)]
                return ProjectTask(top, columns=[*key, *[agg.projection() for agg in requested]])
            return top
        return task

    @staticmethod
    def cleanup_output_column_names(task: Task) -> None:
        schema = task.inferred_schema
        if schema is None:
            raise AssertionError("schema not inferred")
        if not any("." in name for name, _ in schema):
            return
        renamed = [Col(name).alias(name.rsplit(".", 1)[-1]) for name, _ in schema]
        task.parent_task = ProjectTask(task.parent_task, columns=renamed)
        clean = [(col.name, col_type) for col, (_, col_type) in zip(renamed, schema, strict=True)]
        task.parent_task.inferred_schema = clean
        task.inferred_schema = clean

    @staticmethod
    def check_sort_is_last(task: Task, *, top: bool = True) -> None:
        """ORDER BY / LIMIT orders the query's RESULT: the engine runs it once, on the finished rows, so a SortTask
        anywhere but on top of the chain has no meaning here."""
        node: Task | None = task
        while node is not None and type(node) is not VoidTask:
            if type(node) is SortTask and not top and node.windows:
                raise ValueError("a window item (OVER) reads the query's result rows: window() / QUALIFY must be the last "
                                 "operation, not below a join, an aggregate or another operation")
            if type(node) is SortTask and not top:
                raise ValueError("DISTINCT / ORDER BY / LIMIT must be the last operation")
            if type(node) in (BroadcastHashJoinTask, SemiJoinTask):
                PhysicalPlan.check_sort_is_last(node.right_side_task, top=False)
            top = False
            node = node.parent_task

    @staticmethod
    def generate_physical_plan(full_task: Task) -> "PhysicalPlan":
        PhysicalPlan.check_sort_is_last(full_task)
        # planning rewrites nodes in place; work on a copy so the caller's DataFrame stays reusable
        root: Task = WriteToLocalFileTask(deepcopy(full_task))
        PhysicalPlan.infer_schema(root)
        root = PhysicalPlan.expand_tasks(root)
        PhysicalPlan.infer_schema(root)
        PhysicalPlan.cleanup_output_column_names(root)
        stages: list[Stage] = []
        _execution_order(_cut(root), stages)
        for i, stage in enumerate(stages):
            stage.late_initialize(str(i))
        return PhysicalPlan(stages)

    def explain(self) -> None:
        for i, stage in enumerate(self.stages):
            print("Stage", i)  # noqa: T201
            stage.explain()
            print("-" * 10)  # noqa: T201
