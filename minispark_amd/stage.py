"""Host side of the stage-level C ABI (include/hipspark.h, csrc/hs_engine.hip): lower a GROUP BY query into the plan
blob, and a thin handle over ``hs_engine_* / hs_table_* / hs_stage_* / hs_result_*``.

No torch, no :class:`minispark_amd.device.Device`: this is the whole host a cgo / JNI / FFI binding has to reproduce
 - everything else (BlockFile reading, buffers, geometry, retries, replay, hand-over) happens
behind the ABI.  The query shape it covers is the hot path's: ``table -> [filter]* -> group_by(col).agg(...)``, i.e. the
reference's two stages [Load -> Filter* -> Aggregate(before) -> shuffle] + [shuffle -> Aggregate(after) -> (Project) ->
result] (plan.py:182-204); round 3: a SELECT in front of the GROUP BY (its columns inlined, a computed INTEGER key
materialised by the library), and any number of groups per block the on-chip tiers hold; round 5: a join whose rows go to
the result file (lower_join_select_stage_plan / NativeJoinSelectStage) and any join feeding a GROUP BY
(lower_join_group_stage_plan / NativeJoinGroupStage).
"""

from __future__ import annotations

import copy
import ctypes as C
from datetime import datetime
from pathlib import Path
from typing import Any

import numpy as np

from . import constants
from . import hipspark as hs
from .constants import ColumnType, Row, Schema
from .io import BlockFile, StrCol, rows_from_raw
from .lowering import ProgramBuilder, lower_aggregate, lower_finish, unalias
from .plan import PhysicalPlan
from .sql import Col

_FILE_KIND = {ColumnType.INTEGER: hs.I32, ColumnType.FLOAT: hs.F32, ColumnType.TIMESTAMP: hs.I64, ColumnType.STRING: hs.STR}
_TYPE_CODE = {ColumnType.INTEGER: 0, ColumnType.STRING: 1, ColumnType.FLOAT: 2, ColumnType.TIMESTAMP: 3}
_NP = {hs.I32: np.int32, hs.F32: np.float32, hs.I64: np.int64}


class StageUnsupported(NotImplementedError):
    """The query is not of the shape the stage-level path runs (the engine's general path takes it)."""


def _cls(obj: Any) -> str:
    return type(obj).__name__


def _substitute(node: Any, defs: dict[str, Any] | None) -> Any:
    """``node`` over the columns a ProjectTask produced -> the same expression over the table's columns (every projected
    name replaced by its definition): the projection is a pure function of the row (reference tasks.py:32-35,
    sql.py:262-266) and its values are not stored in between, so inlining it gives the same values."""
    if defs is None:
        return node
    name = _cls(node)
    if name == "AliasColumn":
        return _substitute(node.original_col, defs)
    if name in ("Col", "SchemaCol"):
        if node.name not in defs:
            raise ValueError(f'Column "{node.name}" not found in schema {list(defs)}')
        return defs[node.name]
    if name == "Lit":
        return node
    if name == "LikeColumn":
        return type(node)(_substitute(node.original_col, defs), node.pattern)
    if name == "BinaryOperatorColumn":
        return type(node)(_substitute(node.left_side, defs), _substitute(node.right_side, defs), node.operator)
    if name == "CaseColumn":
        return type(node)(_substitute(node.condition, defs), _substitute(node.then_col, defs), _substitute(node.else_col, defs))
    if name == "DatePartColumn":
        return type(node)(node.part, _substitute(node.original_col, defs))
    if name == "DateTruncColumn":
        return type(node)(node.unit, _substitute(node.original_col, defs))
    raise StageUnsupported(f"{name} over a projected column")


_DATE_PART_BITS = {"year": 19, "quarter": 3, "month": 4, "day": 5, "hour": 5, "minute": 6, "second": 6, "dayofweek": 3,
                   "dayofyear": 9}


def _int_bits(node: Any, schema: Schema) -> int | None:
    """b with |value| <= 2**b for an INTEGER-valued expression that cannot raise on ANY row (no division by a column,
    no overflow of the 64-bit cells), else None.  A computed GROUP BY key is evaluated over all rows of the table -
    also the ones the WHERE drops - which is only the reference's behaviour when nothing can go wrong on those rows."""
    name = _cls(node)
    if name == "AliasColumn":
        return _int_bits(node.original_col, schema)
    if name in ("Col", "SchemaCol"):
        types = dict(schema)
        return 31 if types.get(node.name) == ColumnType.INTEGER else None
    if name == "Lit":
        return node.value.bit_length() if type(node.value) is int else None
    if name == "DatePartColumn":
        # total over i64 (no flag, no exception), so only the argument's type is asked for: a TIMESTAMP column, a datetime
        # literal or a DATE_TRUNC of one.  |year| <= 292 278 < 2**19; the other parts are bounded by their calendar
        arg = unalias(node.original_col)
        while _cls(arg) == "DateTruncColumn":
            arg = unalias(arg.original_col)
        if _cls(arg) in ("Col", "SchemaCol"):
            if dict(schema).get(arg.name) != ColumnType.TIMESTAMP:
                return None
        elif _cls(arg) != "Lit" or type(arg.value) is not datetime:
            return None
        return _DATE_PART_BITS[node.part]
    if name != "BinaryOperatorColumn":
        return None
    op = node.operator.__name__
    left = _int_bits(node.left_side, schema)
    if left is None:
        return None
    if op in ("mod", "floordiv"):
        right = unalias(node.right_side)
        if _cls(right) != "Lit" or type(right.value) is not int or right.value == 0:
            return None
        return abs(right.value).bit_length() if op == "mod" else left + 1
    right_bits = _int_bits(node.right_side, schema)
    if right_bits is None:
        return None
    bits = {"add": max(left, right_bits) + 1, "sub": max(left, right_bits) + 1, "mul": left + right_bits}.get(op)
    return bits if bits is not None and bits <= 62 else None


COMPUTED_KEY = "__hs_computed_key"
GROUP_KEY = "__hs_group_key"


def raise_for_flags(flags: int) -> None:
    """Data-dependent failures surface as the exceptions the reference's Python raises (same table as Device)."""
    if flags & hs.FLAG_DIV_ZERO:
        raise ZeroDivisionError("division by zero")
    if flags & hs.FLAG_INT_OVERFLOW:
        raise OverflowError("int too big to convert")
    if flags & hs.FLAG_FLT_OVERFLOW:
        raise OverflowError("float too large to pack with f format")
    if flags & hs.FLAG_TYPE_ASSERT:
        raise AssertionError("FLOAT column holds int")
    if flags & hs.FLAG_BAD_PROGRAM:
        raise RuntimeError("internal error: device interpreter rejected the program")


def read_result_file(path: Path | str) -> list[Row]:
    return list(BlockFile(Path(path)).read_data_rows())


# ---- what the five lowerings share ---------------------------------------------------------------------------------------
def _plan_of(full_task: Any, plan: Any) -> list:
    """The stages of ``plan``, or of the physical plan of ``full_task`` when none is given."""
    stages = list((plan if plan is not None else PhysicalPlan.generate_physical_plan(full_task)).stages)
    for stage in stages:
        if _cls(stage.producer) == "SemiJoinTask":
            # (no stage blob describes a key set; the engine runs it through Device.semi_select: DESIGN.md 4.4j)
            raise StageUnsupported("a LEFT SEMI / LEFT ANTI join")
        for task in stage.consumers:
            if _cls(task) == "MarkFirstTask":
                # (the marks are a pass over the whole batch in front of the scan: DESIGN.md 4.4e)
                raise StageUnsupported("COUNT(DISTINCT)")
            if _cls(task) == "AggregateTask" and task.group_by_column is None:
                # (the stage blobs describe a key column; the engine runs this form through hs_agg_scalar)
                raise StageUnsupported("an aggregate without GROUP BY")
            if _cls(task) == "UnpackKeyTask" or (_cls(task) == "AggregateTask" and _cls(task.group_by_column) == "KeyTupleCol"):
                # (the stage blobs describe ONE key column of the table; the engine packs the tuple first: DESIGN.md 4.4c)
                raise StageUnsupported("GROUP BY over several columns")
    return stages


def _partial_of(consumers: Any, where: str, before: Any) -> Any:
    """The partial aggregate of the producing stage, or None.  ``before(task)`` takes every FilterTask / ProjectTask in front
    of it (what they mean differs per stage) and answers whether the stage holds such a task there."""
    partial = None
    for task in consumers:
        if partial is None and _cls(task) in ("FilterTask", "ProjectTask") and before(task):
            continue
        if partial is None and _cls(task) == "AggregateTask" and task.before_shuffle:
            partial = task
        else:
            raise StageUnsupported(f"{_cls(task)} in the {where} stage")
    return partial


def _aggregate_tail(partial: Any, final: Any, several_projections: bool = False) -> tuple[Any, list | None, Schema]:
    """The final stage of a GROUP BY: the merging aggregate, then at most a projection (``several_projections``: any number in
    a row, folded into one by inlining each one's names into the next) -> (merge task, projected columns or None, result schema)."""
    consumers = list(final.consumers)
    if partial is None or not consumers or _cls(consumers[0]) != "AggregateTask" or consumers[0].before_shuffle:
        raise StageUnsupported("no partial / final aggregate pair")
    if several_projections:
        if any(_cls(t) != "ProjectTask" for t in consumers[1:]):
            raise StageUnsupported("more than a projection after the final aggregate (HAVING)")
    elif len(consumers) > 2 or (len(consumers) == 2 and _cls(consumers[1]) != "ProjectTask"):
        raise StageUnsupported("more than a projection after the final aggregate")
    project, prev = None, None
    for t in consumers[1:]:
        defs = {n: unalias(c) for (n, _), c in zip(prev.inferred_schema, project)} if project is not None else None
        project, prev = [_substitute(c, defs) for c in t.columns], t
    return consumers[0], project, list(final.writer.inferred_schema)


def _where_program(schema: Schema, conds: list) -> Any:
    """The conjunction of ``conds`` as one program with a mask output over ``schema``'s columns, or None without conditions."""
    if not conds:
        return None
    cond = conds[0]
    for extra in conds[1:]:
        cond = cond & extra
    kinds = [_FILE_KIND[t] for _, t in schema]
    fb = ProgramBuilder(schema, kinds)
    if fb.emit_out(0, cond) != "B":  # a number as a condition: true where it is not 0
        fb = ProgramBuilder(schema, kinds)
        fb.emit_out(0, cond != 0)
    return fb.finish()


def _set_program(blob: Any, n_field: str, ids_field: str, prog_field: str, prog: Any) -> None:
    """A program and the table columns behind its slots -> the three fields of a plan blob that hold them."""
    setattr(blob, n_field, len(prog.columns))
    ids = getattr(blob, ids_field)
    for slot, idx in enumerate(prog.columns):
        ids[slot] = idx
    setattr(blob, prog_field, prog.to_struct())


def _set_outputs(blob: Any, out_schema: Schema) -> None:
    """Result column types and names.  The writer's schema never holds an ``alias.`` prefix: the planner's last rewrite strips
    them (plan.py cleanup_output_column_names), so names go in as they are."""
    for o, (name, ctype) in enumerate(out_schema):
        blob.out_types[o] = _TYPE_CODE[ctype]
        blob.out_names[o].value = name.encode()[:63]


def _fill_aggregate(blob: Any, low: Any, kinds: list, merge: Any, project: list | None, out_schema: Schema, col_ids: list,
                    caps: tuple[int, int]) -> None:
    """The part every aggregating plan blob ends with: column slots, key slot, starting capacities, the partial aggregate's
    program and spec, the final merge's folds and projection program, result types and names.  ``col_ids``: per slot of the
    program what the stage reads there (a table column, or -1 for the column the stage makes itself)."""
    acc_kinds = [hs.I32 if is_int else hs.F32 for is_int in low.acc_is_int]
    key_idx = low.program.columns[low.key_slot]
    fin, fin_prog, _ = lower_finish(low.agg_to_acc, acc_kinds, kinds[key_idx], merge.agg_columns, merge.inferred_schema, project,
                                    out_schema)
    blob.n_cols = len(col_ids)
    for slot, idx in enumerate(col_ids):
        blob.col_ids[slot] = idx
    blob.key_slot = low.key_slot
    blob.group_cap, blob.merge_cap = caps
    blob.prog = low.program.to_struct()
    blob.spec = low.spec()
    blob.fin = fin
    if fin_prog is not None:
        blob.fin_prog = fin_prog
    _set_outputs(blob, out_schema)


def lower_stage_plan(full_task: Any, plan: Any = None) -> tuple[hs.hs_stage_plan, Path, Schema]:
    """Task tree (reference or this package's classes) -> (plan blob, table path, result schema)."""
    stages = _plan_of(full_task, plan)
    if len(stages) != 2:
        raise StageUnsupported(f"{len(stages)} stages: the stage-level path runs scan + GROUP BY queries")
    scan, final = (stages if _cls(stages[0].producer) == "LoadTableBlockTask" else stages[::-1])
    if _cls(scan.producer) != "LoadTableBlockTask" or _cls(final.producer) != "LoadShuffleFilesTask":
        raise StageUnsupported("not a scan stage feeding a final stage")
    filters: list = []
    defs: dict[str, Any] | None = None  # after a ProjectTask: projected name -> its expression over the table's columns

    def before(task: Any) -> bool:
        nonlocal defs
        if _cls(task) == "FilterTask":
            filters.append(_substitute(task.condition, defs))
            return True
        names = [n for n, _ in task.inferred_schema]
        if len(names) != len(task.columns) or any(getattr(unalias(c), "name", "") == "*" for c in task.columns):
            raise StageUnsupported("SELECT * in the scan stage")
        defs = {n: _substitute(unalias(c), defs) for n, c in zip(names, task.columns)}
        return True

    partial = _partial_of(scan.consumers, "scan", before)
    merge, project, out_schema = _aggregate_tail(partial, final)

    table_schema = list(scan.producer.inferred_schema)
    kinds = [_FILE_KIND[t] for _, t in table_schema]
    group_by, agg_columns = partial.group_by_column, list(partial.agg_columns)
    key_program = None
    if defs is not None:  # the projection, inlined (values are not stored between a ProjectTask and its consumer)
        group_by = _substitute(group_by, defs)
        for i, agg in enumerate(agg_columns):
            agg_columns[i] = copy.copy(agg)
            agg_columns[i].original_col = _substitute(agg.original_col, defs)
        if _cls(unalias(group_by)) not in ("Col", "SchemaCol"):
            # GROUP BY a computed column: materialised per run by the library as a stored INTEGER column next to the table's
            bits = _int_bits(group_by, table_schema)
            if bits is None or bits > 30:
                raise StageUnsupported("a computed GROUP BY key must be an INTEGER expression that provably fits the stored type")
            kb = ProgramBuilder(table_schema, kinds)
            if kb.emit_out(0, group_by) != "I":
                raise StageUnsupported("a computed GROUP BY key must be INTEGER-valued")
            key_program = kb.finish()
            table_schema = table_schema + [(COMPUTED_KEY, ColumnType.INTEGER)]
            kinds = kinds + [hs.I32]
            group_by = Col(COMPUTED_KEY)
    low = lower_aggregate(table_schema, kinds, filters, group_by, agg_columns)
    if low.numeric_slots > hs.HS_FUSED_COLS:
        raise StageUnsupported(f"more than {hs.HS_FUSED_COLS} numeric columns")
    computed = len(table_schema) - 1 if key_program is not None else -1  # the column the library makes: id -1 in the blob
    blob = hs.hs_stage_plan()
    blob.version = hs.HS_STAGE_PLAN_VERSION
    _fill_aggregate(blob, low, kinds, merge, project, out_schema, [-1 if idx == computed else idx for idx in low.program.columns],
                    (4, 16))
    if key_program is not None:
        if any(idx == computed for slot, idx in enumerate(low.program.columns) if slot != low.key_slot):
            raise AssertionError("the computed key column is read by name only as the key")
        blob.key_computed = 1
        _set_program(blob, "n_kcols", "kcol_ids", "key_prog", key_program)
    return blob, Path(scan.producer.file_path), out_schema


def _join_group_stages(stages: list) -> tuple[Any, Any]:
    """[scan, scan, join -> partial aggregate, final] -> (the join's stage, the final stage)."""
    join = next((st for st in stages if _cls(st.producer) == "BroadcastHashJoinTask"), None)
    final = next((st for st in stages if _cls(st.producer) == "LoadShuffleFilesTask" and _cls(st.writer) == "WriteToLocalFileTask"), None)
    if join is None or final is None or len(stages) != 4 or len(join.dependencies) != 2:
        raise StageUnsupported("not a [scan, scan, join -> partial aggregate, final] plan")
    return join, final


def _set_join(blob: Any, build_key_col: int, probe_key_col: int, n_parts: int | None) -> None:
    blob.build_key_col, blob.probe_key_col = build_key_col, probe_key_col
    blob.n_parts = n_parts if n_parts is not None else constants.SHUFFLE_PARTITIONS


def lower_join_stage_plan(full_task: Any, plan: Any = None, n_parts: int | None = None) -> tuple[hs.hs_join_stage_plan, Path, Path, Schema]:
    """orders JOIN lineitem ... GROUP BY (BASELINE config 4's shape) -> (plan blob of the native JOIN stage, build table path,
    probe table path, result schema).  The reference plans such a query as four stages: shuffle of
    either input by the join key, [join -> partial aggregate -> shuffle], final; the native stage runs the last two
    over the tables themselves, with the JoinJob of a row given by hash(key) % n_parts (plan.py:99-109, tasks.py:362).
    This stage reads the tables under their FILE schema (names prefixed by the alias) and takes no WHERE or renaming
    between a table and the join, so it does not go through the scopes of the two general join stages below."""
    join, final = _join_group_stages(_plan_of(full_task, plan))
    sides = []
    for dep in join.dependencies:  # the two inputs: plain scans, at most a projection that only selects columns
        if _cls(dep.producer) != "LoadTableBlockTask":
            raise StageUnsupported("a join input is not a table scan")
        for task in dep.consumers:
            if _cls(task) != "ProjectTask" or any(_cls(unalias(c)) not in ("Col", "SchemaCol") for c in task.columns):
                raise StageUnsupported(f"{_cls(task)} between a table and the join")
        sides.append(dep.producer)
    build, probe = sides
    filters: list = []

    def before(task: Any) -> bool:  # a WHERE stays in the aggregate's program; a projection after the join is not taken
        if _cls(task) == "FilterTask":
            filters.append(task.condition)
        return _cls(task) == "FilterTask"

    partial = _partial_of(join.consumers, "join", before)
    merge, project, out_schema = _aggregate_tail(partial, final)

    def table_names(producer: Any) -> list[str]:
        prefix = f"{producer.alias}." if getattr(producer, "alias", "") else ""
        return [prefix + n for n, _ in BlockFile(Path(producer.file_path)).file_schema]

    bnames, pnames = table_names(build), table_names(probe)
    bschema, pschema = list(BlockFile(Path(build.file_path)).file_schema), list(BlockFile(Path(probe.file_path)).file_schema)
    lname, rname = join.producer.left_key.name, join.producer.right_key.name
    if lname not in bnames or rname not in pnames:
        raise StageUnsupported("join keys are not plain columns of the two tables")
    # the aggregate's view: every probe-side column under its name + the build-side columns it names
    used = set()
    for expr in [*filters, partial.group_by_column, *[a.original_col for a in partial.agg_columns]]:
        used.update(c.name for c in expr.all_nested_columns if _cls(c) in ("Col", "SchemaCol"))
    wanted_build = sorted(n for n in used if n in bnames and n not in pnames)
    if len(wanted_build) > 1:
        raise StageUnsupported("the aggregate reads more than one build-side column")
    payload = wanted_build[0] if wanted_build else None
    if payload is not None and any(c.name == payload for f in filters for c in f.all_nested_columns if _cls(c) in ("Col", "SchemaCol")):
        raise StageUnsupported("a predicate on the build-side column")  # it exists as a table byte only
    schema = [(n, t) for n, (_, t) in zip(pnames, pschema)]
    if payload is not None:
        if bschema[bnames.index(payload)][1] != ColumnType.STRING:
            raise StageUnsupported("the build-side column must be a STRING column")
        schema.append((payload, ColumnType.STRING))
    kinds = [_FILE_KIND[t] for _, t in schema]
    # the payload is lowered as a dictionary-coded string (one code byte): the dictionary itself is built natively, its
    # contents do not matter to the program as long as no predicate looks inside the strings
    dicts = [None] * len(pnames) + ([(b"",)] if payload is not None else [])
    low = lower_aggregate(schema, kinds, filters, partial.group_by_column, partial.agg_columns, dicts)
    if low.program.code_columns:
        raise StageUnsupported("a predicate on dictionary codes")
    if low.numeric_slots >= hs.HS_FUSED_COLS:
        raise StageUnsupported(f"more than {hs.HS_FUSED_COLS - 1} column slots")
    blob = hs.hs_join_stage_plan()
    blob.version = hs.HS_JOIN_STAGE_PLAN_VERSION
    _set_join(blob, bnames.index(lname), pnames.index(rname), n_parts)
    blob.build_payload_col = bnames.index(payload) if payload is not None else -1
    _fill_aggregate(blob, low, kinds, merge, project, out_schema, [idx if idx < len(pnames) else -1 for idx in low.program.columns],
                    (4, 16))
    return blob, Path(build.file_path), Path(probe.file_path), out_schema


def lower_select_stage_plan(full_task: Any, plan: Any = None) -> tuple[hs.hs_select_stage_plan, Path, Schema]:
    """table -> [filter]* -> [select] (one stage, rows to the result file) -> (plan blob of the native SELECT / WHERE stage,
    table path, result schema)."""
    stages = _plan_of(full_task, plan)
    if len(stages) != 1 or _cls(stages[0].producer) != "LoadTableBlockTask" or _cls(stages[0].writer) != "WriteToLocalFileTask":
        raise StageUnsupported("not a one-stage scan to the result file")
    stage = stages[0]
    filters, project = [], None
    for task in stage.consumers:
        if _cls(task) == "FilterTask" and project is None:
            filters.append(task.condition)
        elif _cls(task) == "ProjectTask" and project is None:
            project = task
        else:
            raise StageUnsupported(f"{_cls(task)} after the projection")
    out_schema = list(stage.writer.inferred_schema)
    table_schema = list(stage.producer.inferred_schema)
    names = [n for n, _ in table_schema]
    blob = hs.hs_select_stage_plan()
    blob.version = hs.HS_SELECT_STAGE_PLAN_VERSION
    where = _where_program(table_schema, filters)
    if where is not None:
        _set_program(blob, "n_cols", "col_ids", "filter", where)
    if project is None:  # every column as it is
        if len(out_schema) != len(table_schema):
            raise StageUnsupported("writer schema differs from the table's")
        srcs = list(range(len(table_schema)))
    else:
        pb = ProgramBuilder(table_schema, [_FILE_KIND[t] for _, t in table_schema])
        srcs, n_prog = [], 0
        for o, col in enumerate(project.columns):
            bare = unalias(col)
            if _cls(bare) in ("Col", "SchemaCol"):
                if bare.name not in names:
                    raise ValueError(f'Column "{bare.name}" not found in schema {table_schema}')
                srcs.append(names.index(bare.name))
                continue
            if pb.string_tag(bare):
                raise StageUnsupported("string expression in the projection")
            if n_prog >= hs.HS_MAX_OUTS:
                raise StageUnsupported("too many computed columns")
            tag = pb.emit_out(n_prog, col)
            if tag == "B":
                raise AssertionError("a comparison cannot be selected as a column (the reference has no BOOL type)")
            want = out_schema[o][1]
            if (tag, want) not in (("F", ColumnType.FLOAT), ("I", ColumnType.INTEGER)):
                raise StageUnsupported(f"computed column of tag {tag} stored as {want}")
            blob.project_kinds[n_prog] = hs.F64 if tag == "F" else hs.I64
            srcs.append(-1 - n_prog)
            n_prog += 1
        if n_prog:
            _set_program(blob, "n_pcols", "pcol_ids", "project", pb.finish())
    if len(srcs) != len(out_schema) or len(srcs) > hs.HS_FINISH_MAX_OUT:
        raise StageUnsupported("result schema does not match the selected columns")
    blob.n_out = len(srcs)
    for o, src in enumerate(srcs):
        blob.out_src[o] = src
    _set_outputs(blob, out_schema)
    return blob, Path(stage.producer.file_path), out_schema


# ---- the two general join stages: every column name in scope -> (side, table column); side 0 = build (the join's left
# input), 1 = probe ----------------------------------------------------------------------------------------------------------
def _walk_names(node: Any) -> list[str]:
    """Column names an expression reads (plain columns, through aliases, LIKE and operators)."""
    name = _cls(node)
    if name in ("Col", "SchemaCol"):
        return [node.name]
    if name == "Lit":
        return []
    if name in ("AliasColumn", "LikeColumn"):
        return _walk_names(node.original_col)
    if name == "BinaryOperatorColumn":
        return _walk_names(node.left_side) + _walk_names(node.right_side)
    if name == "CaseColumn":
        return _walk_names(node.condition) + _walk_names(node.then_col) + _walk_names(node.else_col)
    if name in ("DatePartColumn", "DateTruncColumn"):
        return _walk_names(node.original_col)
    raise StageUnsupported(f"{name} in a join predicate")


def _conjuncts(node: Any) -> list[Any]:
    bare = unalias(node)
    if _cls(bare) == "BinaryOperatorColumn" and bare.operator.__name__ == "and_":
        return _conjuncts(bare.left_side) + _conjuncts(bare.right_side)
    return [node]


def _push_filter(condition: Any, scope: dict, filters: tuple, table_names: list, cross: list | None = None) -> None:
    """Every conjunct of a WHERE -> over the table columns of the one side it reads -> that side's filters.  A conjunct
    over both sides goes to ``cross`` as it is (over the names in scope) when given, else it is refused."""
    for conj in _conjuncts(condition):
        names = _walk_names(conj)
        missing = [n for n in names if n not in scope]
        if missing:
            raise ValueError(f'Column "{missing[0]}" not found in schema {list(scope)}')
        sides = {scope[n][0] for n in names}
        if len(sides) > 1 and cross is not None:
            cross.append(conj)
            continue
        if len(sides) > 1:
            raise StageUnsupported("a WHERE conjunct over both sides of the join")
        side = sides.pop() if sides else 1
        defs = {n: Col(table_names[scope[n][0]][scope[n][1]]) for n in names}
        filters[side].append(_substitute(conj, defs))


def _rename_only(task: Any, scope: dict, what: str) -> tuple[dict, list]:
    """A projection that only passes columns through or renames them -> (the scope after it, what each of its columns reads).
    A repeated name reads its first column, as the engine's lookup does."""
    new, refs = {}, []
    for (n, _), c in zip(task.inferred_schema, task.columns):
        bare = unalias(c)
        if _cls(bare) not in ("Col", "SchemaCol") or bare.name == "*" or bare.name not in scope:
            raise StageUnsupported(f"a computed column {what}")
        refs.append(scope[bare.name])
        new.setdefault(n, scope[bare.name])
    return new, refs


def _join_sides(join: Any) -> tuple[list, list, list, tuple]:
    """The two inputs of a join, each a table scan -> [(producer, table schema)] per side, the tables' column names, the scope
    each side hands to the join (a WHERE in a scan stage is pushed as it is, a projection may select / rename), and the
    filters pushed so far per side."""
    tables, scope_per_side, filters = [], [], ([], [])
    for dep in join.dependencies:
        if _cls(dep.producer) != "LoadTableBlockTask":
            raise StageUnsupported("a join input is not a table scan")
        tables.append((dep.producer, list(dep.producer.inferred_schema)))
    table_names = [[n for n, _ in schema] for _, schema in tables]
    for side, dep in enumerate(join.dependencies):
        scope = {n: (side, i) for i, n in enumerate(table_names[side])}
        for task in dep.consumers:
            if _cls(task) == "FilterTask":
                _push_filter(task.condition, scope, filters, table_names)
            elif _cls(task) != "ProjectTask":
                raise StageUnsupported(f"{_cls(task)} between a table and the join")
            else:
                scope, _ = _rename_only(task, scope, "between a table and the join")
                if len(scope) != len(task.columns):
                    raise StageUnsupported("a projection that repeats a column name before the join")
        scope_per_side.append(scope)
    return tables, table_names, scope_per_side, filters


def _join_keys(task: Any, scope_per_side: list) -> tuple[int, int]:
    """-> the table columns of the join's keys (build side, probe side)."""
    lname, rname = task.left_key.name, task.right_key.name
    if lname not in scope_per_side[0] or rname not in scope_per_side[1]:
        raise StageUnsupported("join keys are not plain columns of the two inputs")
    return scope_per_side[0][lname][1], scope_per_side[1][rname][1]


def _check_key_types(tables: list, build_key_col: int, probe_key_col: int) -> None:
    ltype, rtype = tables[0][1][build_key_col][1], tables[1][1][probe_key_col][1]
    if ltype != rtype or ltype not in (ColumnType.INTEGER, ColumnType.STRING):
        raise StageUnsupported(f"join keys of kinds {ltype} / {rtype}: both INTEGER or both STRING")


def _lower_side_filters(blob: Any, tables: list, filters: tuple) -> None:
    """The pushed-down WHERE of either side -> its filter program and column slots in a join plan blob."""
    for side, fields in enumerate((("n_bcols", "bcol_ids", "build_filter"), ("n_pcols", "pcol_ids", "probe_filter"))):
        prog = _where_program(tables[side][1], filters[side])
        if prog is None:
            continue
        if len(prog.columns) > hs.HS_MAX_COLS:
            raise StageUnsupported(f"a WHERE over more than {hs.HS_MAX_COLS} columns")
        _set_program(blob, *fields, prog)


def lower_join_select_stage_plan(full_task: Any, plan: Any = None,
                                 n_parts: int | None = None) -> tuple[hs.hs_join_select_stage_plan, Path, Path, Schema]:
    """[scan, scan, join -> result file] (a JoinJob whose rows go to the result file, jobs.py:45-79) -> (plan blob of the
    native JOIN-to-rows stage, build table path, probe table path, result schema).  Projections may only pass columns through
    or rename them; every WHERE conjunct must read one side only and is pushed to that side's scan (the join keeps the order
    of the rows that survive, so the result and its order do not change)."""
    stages = _plan_of(full_task, plan)
    join = next((st for st in stages if _cls(st.producer) == "BroadcastHashJoinTask"), None)
    if join is None or len(stages) != 3 or len(join.dependencies) != 2 or _cls(join.writer) != "WriteToLocalFileTask":
        raise StageUnsupported("not a [scan, scan, join -> result file] plan")
    tables, table_names, scope_per_side, filters = _join_sides(join)
    build_key_col, probe_key_col = _join_keys(join.producer, scope_per_side)
    scope = {**scope_per_side[1], **scope_per_side[0]}  # a name on both sides reads the build side's, as the engine's lookup does
    order = list(scope_per_side[0].values()) + list(scope_per_side[1].values())
    for t in join.consumers:
        if _cls(t) == "FilterTask":
            _push_filter(t.condition, scope, filters, table_names)
        elif _cls(t) == "ProjectTask":
            scope, order = _rename_only(t, scope, "after the join")
        else:
            raise StageUnsupported(f"{_cls(t)} after the join (a join feeding an aggregate is hs_join_stage)")
    out_schema = list(join.writer.inferred_schema)
    if len(order) != len(out_schema):
        raise StageUnsupported("result schema does not match the joined columns")
    if len(order) > hs.HS_FINISH_MAX_OUT:
        raise StageUnsupported(f"more than {hs.HS_FINISH_MAX_OUT} result columns")
    _check_key_types(tables, build_key_col, probe_key_col)
    blob = hs.hs_join_select_stage_plan()
    blob.version = hs.HS_JOIN_SELECT_STAGE_PLAN_VERSION
    _set_join(blob, build_key_col, probe_key_col, n_parts)
    _lower_side_filters(blob, tables, filters)
    blob.n_out = len(order)
    for o, ((_, ctype), (side, col)) in enumerate(zip(out_schema, order)):
        if tables[side][1][col][1] != ctype:
            raise StageUnsupported("a result column changes its type")
        blob.out_side[o], blob.out_col[o] = side, col
    _set_outputs(blob, out_schema)
    return blob, Path(tables[0][0].file_path), Path(tables[1][0].file_path), out_schema


def lower_join_group_stage_plan(full_task: Any, plan: Any = None,
                                n_parts: int | None = None) -> tuple[hs.hs_join_group_stage_plan, Path, Path, Schema]:
    """[scan, scan, join -> partial aggregate, final] for any join (keys INTEGER or STRING, duplicates on both sides, columns of
    either side) -> (plan blob of the native JOIN-to-GROUP-BY stage, build table path, probe table path, result schema).
    Projections may only pass columns through or rename them; a WHERE conjunct over one side is pushed to that side's scan,
    one over both sides is the aggregate program's filter.  After the final aggregate at most a projection."""
    join, final = _join_group_stages(_plan_of(full_task, plan))
    tables, table_names, scope_per_side, filters = _join_sides(join)
    build_key_col, probe_key_col = _join_keys(join.producer, scope_per_side)
    scope = {**scope_per_side[1], **scope_per_side[0]}  # a name on both sides reads the build side's, as the engine's lookup does
    cross: list = []

    def before(task: Any) -> bool:
        nonlocal scope
        if _cls(task) == "FilterTask":
            _push_filter(task.condition, scope, filters, table_names, cross)
        else:
            scope, _ = _rename_only(task, scope, "before the aggregate")
        return True

    partial = _partial_of(join.consumers, "join", before)
    merge, project, out_schema = _aggregate_tail(partial, final, several_projections=True)
    _check_key_types(tables, build_key_col, probe_key_col)
    key = unalias(partial.group_by_column)
    if _cls(key) not in ("Col", "SchemaCol") or key.name not in scope:
        raise StageUnsupported("a computed GROUP BY key after the join")
    # the aggregate's view: every name in scope, and the GROUP BY column once more under a name of its own - its slot may
    # hold dictionary codes, which no predicate or argument may read
    where = [*scope.items(), (GROUP_KEY, scope[key.name])]
    schema = [(n, tables[side][1][col][1]) for n, (side, col) in where]
    kinds = [_FILE_KIND[t] for _, t in schema]
    low = lower_aggregate(schema, kinds, cross, Col(GROUP_KEY), partial.agg_columns)
    if len(low.program.columns) > hs.HS_FUSED_COLS:
        raise StageUnsupported(f"more than {hs.HS_FUSED_COLS} column slots")
    blob = hs.hs_join_group_stage_plan()
    blob.version = hs.HS_JOIN_GROUP_STAGE_PLAN_VERSION
    _set_join(blob, build_key_col, probe_key_col, n_parts)
    slots = [where[idx][1] for idx in low.program.columns]  # per slot of the program: (side, table column)
    # (in the parent's order: the final merge is lowered - and may refuse - before the side filters are)
    _fill_aggregate(blob, low, kinds, merge, project, out_schema, [col for _, col in slots], (16, 64))
    for slot, (side, _) in enumerate(slots):
        blob.col_side[slot] = side
    _lower_side_filters(blob, tables, filters)
    return blob, Path(tables[0][0].file_path), Path(tables[1][0].file_path), out_schema


# ---- handles over the library --------------------------------------------------------------------------------------------
class NativeEngine:
    """hs_engine + the tables it has open."""

    def __init__(self, device: int = 0) -> None:
        self.lib = hs.load_library()
        self.handle = C.c_void_p()
        hs.check(self.lib.hs_engine_create(device, C.byref(self.handle)), "hs_engine_create")
        self._tables: dict[tuple, C.c_void_p] = {}

    def table(self, path: Path | str, rank: int = 0, world: int = 1) -> C.c_void_p:
        key = (str(Path(path).resolve()), rank, world)
        if key not in self._tables:
            t = C.c_void_p()
            hs.check(self.lib.hs_table_open(self.handle, key[0].encode(), rank, world, C.byref(t)), "hs_table_open")
            self._tables[key] = t
        return self._tables[key]

    def close(self) -> None:
        for t in self._tables.values():
            self.lib.hs_table_close(t)
        self._tables.clear()
        if self.handle:
            self.lib.hs_engine_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self) -> "NativeEngine":
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()


class _NativeHandle:
    """What the five stage handles share: ``STEM_prepare / _run / _stats / _destroy`` and ``..._result_write_blockfile`` differ
    in the symbol stem only (``hs_join_group_stage`` -> ``hs_join_group_result_write_blockfile``)."""

    stem = ""

    def _call(self, name: str, *args: Any) -> None:
        hs.check(getattr(self.lib, name)(*args), name)

    def _prepare(self, engine: NativeEngine, *tables: Any, extra: tuple = ()) -> None:
        """``self.blob`` and the opened tables -> ``self.handle``."""
        self.engine, self.lib, self.handle = engine, engine.lib, C.c_void_p()
        self._call(f"{self.stem}_prepare", engine.handle, *tables, C.byref(self.blob), C.sizeof(self.blob), *extra,
                   C.byref(self.handle))

    def _run(self, stream: int | None) -> int:
        """One run -> the number of result rows; a data error of the run raises as the reference's Python does."""
        flags, nrows = C.c_uint32(0), C.c_int64(0)
        self._call(f"{self.stem}_run", self.handle, stream, C.byref(flags), C.byref(nrows))
        raise_for_flags(flags.value)
        return int(nrows.value)

    def _write(self, out_path: Path | str, *args: Any) -> Path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        self._call(f"{self.stem.replace('_stage', '_result')}_write_blockfile", self.handle, str(out_path).encode(), *args)
        return Path(out_path)

    def _run_to_file(self, out_path: Path | str, stream: int | None, *args: Any) -> int:
        """One run; its rows go to the BlockFile at out_path (no file for no rows) -> the number of rows."""
        nrows = self._run(stream)
        if nrows:
            self._write(out_path, *args)
        return nrows

    def _stats(self, n: int, which: str = "stats") -> list[int]:
        s = (C.c_int64 * n)()
        self._call(f"{self.stem}_{which}", self.handle, s)
        return [int(v) for v in s]

    def _tier_stats(self) -> dict:
        tier, partial_rows, result_rows, switches = self._stats(4, "tier_stats")
        return {"tier": hs.STAGE_TIERS.get(tier, tier), "partial_rows": partial_rows, "result_rows": result_rows,
                "tier_switches": switches}

    def _set_hbm_tier(self) -> None:
        """Past the on-chip tiers the stage moves to the HBM (radix) tier instead of answering HS_E_LIMIT."""
        self._call(f"{self.stem}_set_hbm_tier", self.handle, 1)

    def close(self) -> None:
        if self.handle:
            getattr(self.lib, f"{self.stem}_destroy")(self.handle)
            self.handle = C.c_void_p()


class NativeStage(_NativeHandle):
    """A prepared query: ``run()`` -> result rows; ``write(path)`` -> the result BlockFile."""

    stem = "hs_stage"

    def __init__(self, engine: NativeEngine, full_task: Any, plan: Any = None, world: int = 1, rank: int = 0,
                 hbm_tier: bool = False) -> None:
        self.blob, self.table_path, self.schema = lower_stage_plan(full_task, plan)
        self._prepare(engine, engine.table(self.table_path, rank, world), extra=(world,))
        if hbm_tier:
            self._set_hbm_tier()

    def run(self, stream: int | None = None) -> list[Row]:
        self._run(stream)
        return list(rows_from_raw(self.schema, self.raw_columns()))

    def raw_columns(self) -> list[Any]:
        cols = (hs.hs_result_col * hs.HS_FINISH_MAX_OUT)()
        n = C.c_int32(0)
        hs.check(self.lib.hs_result_columns(self.handle, cols, hs.HS_FINISH_MAX_OUT, C.byref(n)), "hs_result_columns")
        raw: list[Any] = []
        for o in range(n.value):
            c = cols[o]
            rows, nbytes = int(c.n_rows), int(c.n_rows) * int(c.width)
            buf = np.frombuffer((C.c_uint8 * nbytes).from_address(c.data), dtype=np.uint8).copy() if nbytes else np.zeros(0, np.uint8)
            raw.append(StrCol(np.full(rows, c.width, np.uint8), buf) if c.kind == hs.STR else buf.view(_NP[c.kind]))
        return raw

    def write(self, path: Path | str) -> Path:
        return self._write(path)

    def stats(self) -> dict:
        out = dict(zip(("runs", "replays", "grows", "group_cap", "merge_cap", "chunks"), self._stats(6)))
        out.update(self._tier_stats())
        return out


class NativeSelectStage(_NativeHandle):
    """A prepared select / where query behind the C ABI: ``run(path)`` -> rows (through the result BlockFile the library writes)."""

    stem = "hs_select_stage"

    def __init__(self, engine: NativeEngine, full_task: Any, plan: Any = None) -> None:
        self.blob, self.table_path, self.schema = lower_select_stage_plan(full_task, plan)
        self._prepare(engine, engine.table(self.table_path))

    def run(self, out_path: Path | str, rows_per_block: int | None = None, stream: int | None = None) -> list[Row]:
        return read_result_file(out_path) if self._run_to_file(out_path, stream, rows_per_block or constants.ROWS_PER_BLOCK) else []


class NativeJoinSelectStage(_NativeHandle):
    """A prepared [scan, scan, join -> result file] query behind the C ABI: ``run(path)`` -> rows (through the result BlockFile
    the library writes)."""

    stem = "hs_join_select_stage"

    def __init__(self, engine: NativeEngine, full_task: Any, plan: Any = None, n_parts: int | None = None) -> None:
        self.blob, self.build_path, self.probe_path, self.schema = lower_join_select_stage_plan(full_task, plan, n_parts)
        self._prepare(engine, engine.table(self.build_path), engine.table(self.probe_path))

    def run(self, out_path: Path | str, rows_per_block: int | None = None, stream: int | None = None) -> list[Row]:
        return read_result_file(out_path) if self.run_to_file(out_path, rows_per_block, stream) else []

    def run_to_file(self, out_path: Path | str, rows_per_block: int | None = None, stream: int | None = None) -> int:
        """One run; its rows go to the BlockFile at out_path (no file for no rows) -> the number of rows."""
        return self._run_to_file(out_path, stream, rows_per_block or constants.ROWS_PER_BLOCK)

    def stats(self) -> dict:
        runs, rows, route, n_build, n_probe = self._stats(5)
        return {"runs": runs, "rows": rows, "route": hs.JOIN_ROUTES.get(route, route), "build_rows": n_build, "probe_rows": n_probe}


class NativeJoinStage(_NativeHandle):
    """A prepared join + GROUP BY query behind the C ABI: ``run()`` -> rows (through the result BlockFile the library writes)."""

    stem = "hs_join_stage"

    def __init__(self, engine: NativeEngine, full_task: Any, plan: Any = None) -> None:
        self.blob, self.build_path, self.probe_path, self.schema = lower_join_stage_plan(full_task, plan)
        self._prepare(engine, engine.table(self.build_path), engine.table(self.probe_path))

    def run(self, out_path: Path | str, stream: int | None = None) -> list[Row]:
        return read_result_file(out_path) if self._run_to_file(out_path, stream) else []

    def stats(self) -> dict:
        return dict(zip(("runs", "replays", "grows", "group_cap", "merge_cap", "dictionary", "table_slots", "unit_cap"), self._stats(8)))


class NativeJoinGroupStage(_NativeHandle):
    """A prepared join feeding a GROUP BY (any join keys and columns) behind the C ABI: ``run(path)`` -> rows (through the
    result BlockFile the library writes)."""

    stem = "hs_join_group_stage"

    def __init__(self, engine: NativeEngine, full_task: Any, plan: Any = None, n_parts: int | None = None,
                 hbm_tier: bool = False) -> None:
        self.blob, self.build_path, self.probe_path, self.schema = lower_join_group_stage_plan(full_task, plan, n_parts)
        self._prepare(engine, engine.table(self.build_path), engine.table(self.probe_path))
        if hbm_tier:
            self._set_hbm_tier()

    def run(self, out_path: Path | str, stream: int | None = None) -> list[Row]:
        return read_result_file(out_path) if self._run_to_file(out_path, stream) else []

    def stats(self) -> dict:
        v = self._stats(10)
        return {"runs": v[0], "grows": v[1], "group_cap": v[2], "merge_cap": v[3], "route": hs.JOIN_ROUTES.get(v[4], v[4]),
                "aggregate": hs.JOIN_AGG_ROUTES.get(v[5], v[5]), "pairs": v[6], "build_rows": v[7], "probe_rows": v[8],
                "dictionary": v[9], **self._tier_stats()}
