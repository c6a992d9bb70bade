"""minispark_amd/stage.py, pinned from outside: every plan blob the five ``lower_*_stage_plan`` functions produce and every
refusal they raise, over one corpus of queries, equals the record in tests/golden/stage_plan_blobs.json byte for byte.

The record was written ONCE by ``python -m tests.test_stage_plan_blobs --write`` on the commit before the stage host was
folded into shared helpers (102c67e) and is not regenerated from the code under test: it is what a foreign host's lowering
has to reproduce.  ``--write`` also reports, per function, how many cases lower / refuse and which ``raise`` sites of
stage.py no case reaches.  No GPU: lowering reads the tables' headers only."""

from __future__ import annotations

import ctypes as C
import hashlib
import json
import re
import sys
from pathlib import Path
from typing import Any, Callable

import numpy as np

from minispark_amd import stage
from minispark_amd.constants import ColumnType as T
from minispark_amd.parser import parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col, Functions as F, Lit
from minispark_amd.tasks import AggregateTask, FilterTask, ProjectTask, VoidTask
from minispark_amd import workloads
from tests.conftest import GOLDEN, load_golden
from tests.queries import CASES as QUERY_CASES
from tests.sql_texts import E2E_SQL
from tests.test_gpu_join_dict import _join_queries, _join_tables, _oracle_api
from tests.test_gpu_join_group_stage import _mixed_query, _mixed_tables
from tests.test_gpu_join_select_stage import _str_col, _write

FIXTURE = GOLDEN / "stage_plan_blobs.json"
FUNCTIONS = ["lower_stage_plan", "lower_join_stage_plan", "lower_select_stage_plan", "lower_join_select_stage_plan",
             "lower_join_group_stage_plan"]
MIXED_KINDS = ["string_keys", "cross_side_where", "build_int_key", "probe_timestamp_key", "probe_string_key", "growth",
               "empty_where"]


def _tables(tmp: Path) -> dict[str, str]:
    """Every table the corpus reads: the goldens' (users, orders, the many-groups lineitem, join_group's pair) and generated ones."""
    t = {}
    e2e, jg = load_golden("e2e_join_select")["paths"], load_golden("join_group")["paths"]
    t.update(users=e2e["users"], orders=e2e["orders"], li=load_golden("many_groups")["paths"]["lineitem"],
             jg_orders=jg["orders"], jg_lineitem=jg["lineitem"], q1=load_golden("q1_multiblock")["paths"]["lineitem"])
    for sub in ("join", "mixed", "extra"):
        (tmp / sub).mkdir(parents=True, exist_ok=True)
    t["j_orders"], t["j_lineitem"] = _join_tables(tmp / "join", 300, 2000, seed=21, dup=True)
    t["b"], t["p"] = _mixed_tables(tmp / "mixed", nb=50, np_=200, block_rows=64)
    ones, ints = np.ones(4, np.float32), np.arange(4, dtype=np.int32)
    _write(tmp / "extra" / "fb.bin", [("fk", T.FLOAT), ("g", T.INTEGER)], [ones, ints], 4)
    _write(tmp / "extra" / "fp.bin", [("fk2", T.FLOAT), ("v", T.INTEGER)], [ones, ints], 4)
    wide = [(f"c{i:02d}", T.INTEGER) for i in range(40)]  # more columns than a result file of the stages holds
    _write(tmp / "extra" / "wide.bin", wide, [ints] * 40, 4)
    _write(tmp / "extra" / "wide2.bin", [(f"d{i:02d}", T.INTEGER) for i in range(40)], [ints] * 40, 4)
    _write(tmp / "extra" / "names.bin", [("nk", T.INTEGER), ("bs", T.STRING)], [ints, _str_col([b"x"] * 4)], 4)
    t.update({n: str(tmp / "extra" / f"{n}.bin") for n in ("fb", "fp", "wide", "wide2", "names")})
    return t


def _df(path: str, alias: str = "") -> Any:
    frame = _oracle_api().DataFrame().table(path)
    return frame.alias(alias) if alias else frame


def _uo(t: dict, on: Any = None) -> Any:
    return _df(t["users"], "u").join(_df(t["orders"], "o"), on=on if on is not None else Col("u.user_id") == Col("o.user_id"),
                                     how="inner")


def _bp(t: dict, on: Any = None) -> Any:
    return _df(t["b"]).join(_df(t["p"]), on=on if on is not None else Col("bk") == Col("pk"), how="inner")


def _jg(t: dict) -> Any:  # the byte-table join stage's shape: column-selecting projections, then the join
    o = _df(t["jg_orders"]).select(Col("o_orderkey"), Col("o_orderpriority"), Col("o_totalprice"))
    li = _df(t["jg_lineitem"]).select(Col("l_orderkey"), Col("l_quantity"), Col("l_extendedprice"))
    return o.join(li, on=Col("o_orderkey") == Col("l_orderkey"), how="inner")


def _computed_key(t: dict, key: Any) -> Any:  # tests/test_abi.py, the computed-key frames
    return (_df(t["li"]).filter(Col("l_shipdate") > "1992-03-01")
            .select(key.alias("bucket"), Col("l_extendedprice").alias("price"), (Col("l_tax") * 2).alias("t2"))
            .filter(Col("t2") < 0.15).group_by(Col("bucket")).agg(F.sum(Col("price") * (Lit(1) + Col("t2"))).alias("g"), F.count()))


def _sum_all(names: list[str]) -> list[Any]:
    return [F.sum(Col(n)).alias(f"s_{n}") for n in names]


# ---- plans no query text produces (the planner expands SELECT *, checks names, orders the tasks): edited after planning ----
def _edit(stage_of: Callable[[list], Any], change: Callable[[Any], None]) -> Callable[[Any], Any]:
    def plan_of(task: Any) -> Any:
        plan = PhysicalPlan.generate_physical_plan(task)
        change(stage_of(list(plan.stages)))
        return plan
    return plan_of


def _first(stages: list) -> Any:
    return stages[0]


def _last(stages: list) -> Any:
    return stages[-1]


def _join_stage(stages: list) -> Any:
    return next(st for st in stages if type(st.producer).__name__ == "BroadcastHashJoinTask")


def _append_filter(cond: Any) -> Callable[[Any], None]:
    return lambda st: st.consumers.append(FilterTask(VoidTask(), condition=cond))


def _prepend(task: Any) -> Callable[[Any], None]:
    return lambda st: st.consumers.insert(0, task)


def _star_in_first_projection(st: Any) -> None:
    project = next(c for c in st.consumers if type(c).__name__ == "ProjectTask")
    project.columns = [Col("*"), *project.columns[1:]]


def _unknown_in_first_projection(st: Any) -> None:
    project = next(c for c in st.consumers if type(c).__name__ == "ProjectTask")
    project.columns = [Col("nowhere"), *project.columns[1:]]


def _drop_consumers(st: Any) -> None:
    del st.consumers[:]


def _project(*cols: Any, schema: list | None = None) -> Any:
    return ProjectTask(VoidTask(), columns=list(cols), inferred_schema=schema if schema is not None else [(c.name, T.INTEGER) for c in cols])


# (case name, task builder over the tables, plan editor or None)
def _cases() -> list[tuple[str, Callable[[dict], Any], Callable[[Any], Any] | None]]:
    api = _oracle_api()
    out: list[tuple[str, Callable[[dict], Any], Any]] = []

    def add(name: str, build: Callable[[dict], Any], edit: Any = None) -> None:
        out.append((name, build, edit))

    for case in QUERY_CASES:  # tests/queries.py, each against its golden's tables
        add(f"queries/{case.name}", lambda t, case=case: case.build(api, load_golden(case.name)["paths"]))
    for name in sorted(E2E_SQL):  # tests/sql_texts.py, through the parser
        add(f"sql/{name}", lambda t, name=name: parse_sql(E2E_SQL[name].format(**load_golden(name)["paths"]), object()))
    add("workloads/q1", lambda t: workloads.q1(api, t["q1"]))
    add("workloads/join_group", lambda t: workloads.join_group(api, t["jg_orders"], t["jg_lineitem"]))
    add("computed_key/good", lambda t: _computed_key(t, Col("l_orderkey") % 331 - 100))
    add("computed_key/may_divide_by_zero", lambda t: _computed_key(t, Col("l_orderkey") // Col("l_orderkey")))
    add("computed_key/may_not_fit", lambda t: _computed_key(t, Col("l_orderkey") * 4))
    add("computed_key/square", lambda t: _computed_key(t, Col("l_orderkey") * Col("l_orderkey")))
    add("computed_key/float", lambda t: _computed_key(t, Col("l_tax") * 2))
    add("computed_key/string", lambda t: _computed_key(t, Col("l_returnflag") + "-"))
    for name in ("config4", "filtered_with_build_side_argument", "probe_side_int_key", "filtered_on_the_probe_side", "count_only"):
        add(f"join_dict/{name}", lambda t, name=name: _join_queries(api, t["j_orders"], t["j_lineitem"])[name])
    for kind in MIXED_KINDS:
        add(f"mixed/{kind}", lambda t, kind=kind: _mixed_query(api, t["b"], t["p"], kind))

    # tests/test_join_select_lowering.py, tests/test_gpu_join_select_stage.py
    add("join_select/two_side_where", lambda t: _uo(t).filter((Col("u.age") > 30) & (Col("o.quantity") > 1))
        .select(Col("u.first_name"), Col("o.product")))
    add("join_select/feeds_group_by", lambda t: _uo(t).group_by(Col("u.country")).agg(F.count().alias("n")))
    add("join_select/int_string_keys", lambda t: _uo(t, Col("u.user_id") == Col("o.product")))
    add("join_select/int_timestamp_keys", lambda t: _uo(t, Col("u.user_id") == Col("o.order_date")))
    add("join_select/where_over_both_sides", lambda t: _uo(t).filter(Col("u.age") > Col("o.quantity")).select(Col("u.first_name")))
    add("join_select/computed_column", lambda t: _uo(t).select((Col("o.quantity") * 2).alias("q2")))
    add("join_select/bare_join", lambda t: _uo(t))
    add("join_select/string_keys", lambda t: _bp(t, Col("bt") == Col("pt")).select(Col("bs"), Col("pf")))
    # tests/test_join_group_stage_lowering.py, tests/test_gpu_join_group_stage.py
    add("join_group/computed_before_aggregate", lambda t: _bp(t).select((Col("pf") * 2).alias("x"), Col("bs")).group_by(Col("bs"))
        .agg(F.sum(Col("x")).alias("s")))
    add("join_group/int_string_keys", lambda t: _bp(t, Col("bk") == Col("pt")).group_by(Col("bs")).agg(F.count()))
    add("join_group/too_many_slots", lambda t: _bp(t).filter((Col("bs") != Col("pt")) & (Col("bt") != Col("ps"))).group_by(Col("bs"))
        .agg(F.sum(Col("pf")).alias("a"), F.min(Col("bi")).alias("b"), F.max(Col("pi")).alias("c"), F.sum(Col("bk")).alias("d"),
             F.sum(Col("pk")).alias("e")))
    add("join_group/float_keys", lambda t: _df(t["fb"]).join(_df(t["fp"]), on=Col("fk") == Col("fk2"), how="inner")
        .group_by(Col("g")).agg(F.sum(Col("v")).alias("s")))
    add("join_group/pair_program", lambda t: _df(t["jg_orders"]).join(_df(t["jg_lineitem"]), on=Col("o_orderkey") == Col("l_orderkey"),
                                                                    how="inner")
        .group_by(Col("o_orderpriority")).agg(F.sum(Col("l_quantity") * Col("o_orderkey")).alias("w"), F.count()))
    add("join_group/an_empty_join", lambda t: _df(t["names"]).join(_df(t["fp"]), on=Col("nk") == Col("v"), how="inner")
        .group_by(Col("bs")).agg(F.sum(Col("fk2")).alias("s")))

    # where the five copies differed: aliases, dots, projections in a row, repeated names
    add("alias/build_side_only", lambda t: _df(t["users"], "u").join(_df(t["orders"]), on=Col("u.user_id") == Col("order_id"), how="inner")
        .group_by(Col("u.country")).agg(F.sum(Col("price")).alias("total")))
    add("alias/probe_side_only", lambda t: _df(t["users"]).join(_df(t["orders"], "o"), on=Col("age") == Col("o.order_id"), how="inner")
        .group_by(Col("o.product")).agg(F.max(Col("age")).alias("oldest"), F.count()))
    add("alias/join_rows_probe_side_only", lambda t: _df(t["users"]).join(_df(t["orders"], "o"), on=Col("age") == Col("o.order_id"),
                                                                         how="inner").select(Col("o.product"), Col("first_name")))
    add("alias/scan_group_by", lambda t: _df(t["users"], "u").group_by(Col("u.country")).agg(F.avg(Col("u.age")).alias("u.mean"), F.count()))
    add("alias/scan_select", lambda t: _df(t["users"], "u").filter(Col("u.age") > 25).select(Col("u.first_name"), (Col("u.age") + 1).alias("next")))
    add("dots/result_name_with_a_dot", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.sum(Col("age")).alias("x.total"),
                                                                                            F.count().alias("a.b.c")))
    add("dots/join_result_name_with_a_dot", lambda t: _uo(t).group_by(Col("u.country")).agg(F.sum(Col("o.price")).alias("x.total")))
    add("dots/select_name_with_a_dot", lambda t: _df(t["users"], "u").select(Col("u.age").alias("v.age"), (Col("u.age") * 2).alias("w.x.twice")))
    add("projections/two_after_the_aggregate", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.avg(Col("age")).alias("m"), F.count())
        .select(Col("country").alias("c"), Col("m"), Col("count").alias("n")).select(Col("c"), (Col("m") * 2).alias("m2"), Col("n")))
    add("projections/two_after_the_join_aggregate", lambda t: _uo(t).group_by(Col("u.country"))
        .agg(F.avg(Col("o.price")).alias("m"), F.count()).select(Col("u.country").alias("c"), Col("m"), Col("count").alias("n"))
        .select(Col("c"), (Col("m") * 2).alias("m2"), Col("n")))
    add("projections/one_after_the_join_aggregate", lambda t: _jg(t).group_by(Col("o_orderpriority"))
        .agg(F.avg(Col("l_quantity")).alias("m"), F.count()).select(Col("o_orderpriority").alias("prio"), Col("m")))
    add("projections/filter_after_the_join_aggregate", lambda t: _jg(t).group_by(Col("o_orderpriority"))
        .agg(F.sum(Col("l_quantity")).alias("q")).filter(Col("q") > 10))
    add("projections/having_after_the_scan_aggregate", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.count().alias("n"))
        .filter(Col("n") > 1))
    add("projections/having_then_two", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.count().alias("n"))
        .select(Col("country"), Col("n")).filter(Col("n") > 1).select(Col("country")))
    add("repeated/after_the_join", lambda t: _uo(t).select(Col("u.age").alias("x"), Col("o.quantity").alias("x"), Col("u.first_name")))
    add("repeated/after_the_join_before_group_by", lambda t: _uo(t).select(Col("u.country").alias("x"), Col("o.quantity").alias("x"))
        .group_by(Col("x")).agg(F.count()))
    add("repeated/before_the_join", lambda t: _df(t["users"]).select(Col("user_id").alias("k"), Col("age").alias("k"))
        .join(_df(t["orders"]), on=Col("k") == Col("order_id"), how="inner").select(Col("product")))
    add("renamed/inputs_of_the_join", lambda t: _df(t["users"]).select(Col("user_id").alias("uid"), Col("country").alias("land"))
        .join(_df(t["orders"]).filter(Col("price") > 30).select(Col("user_id").alias("buyer"), Col("price"), Col("quantity")),
              on=Col("uid") == Col("buyer"), how="inner").filter(Col("quantity") > 1).select(Col("land"), Col("price").alias("paid")))
    add("renamed/inputs_of_the_join_group_by", lambda t: _df(t["users"]).select(Col("user_id").alias("uid"), Col("country").alias("land"))
        .join(_df(t["orders"]).filter(Col("price") > 30).select(Col("user_id").alias("buyer"), Col("price"), Col("quantity")),
              on=Col("uid") == Col("buyer"), how="inner").filter((Col("quantity") > 1) & (Col("price") > Col("uid")))
        .select(Col("land").alias("l2"), Col("price"), Col("uid")).group_by(Col("l2")).agg(F.sum(Col("price") * Col("uid")).alias("w")))
    add("renamed/type_changes_at_the_writer", lambda t: _uo(t).select(Col("u.age"), Col("o.product")),
        _edit(_last, lambda st: setattr(st.writer, "inferred_schema", [("age", T.FLOAT), ("product", T.STRING)])))

    # the remaining refusals, one case each
    add("scan/no_aggregate_pair", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.count()), _edit(_first, _drop_consumers))
    add("scan/not_a_scan_feeding_a_final_stage", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.count()),
        _edit(_last, lambda st: setattr(st, "producer", VoidTask())))
    add("scan/filter_after_the_partial_aggregate", lambda t: _df(t["users"]).group_by(Col("country")).agg(F.count()),
        _edit(_first, _append_filter(Col("count") > 1)))
    add("scan/star_left_in_the_projection", lambda t: _df(t["users"]).select(Col("country"), Col("age")).group_by(Col("country")).agg(F.count()),
        _edit(_first, _star_in_first_projection))
    add("scan/unknown_name_over_a_projection", lambda t: _df(t["users"]).select(Col("country"), Col("age")).filter(Col("age") > 1)
        .group_by(Col("country")).agg(F.count()), _edit(_first, lambda st: setattr(st.consumers[1], "condition", Col("nowhere") > 1)))
    add("scan/aggregate_over_a_projection", lambda t: _df(t["users"]).select(Col("country"), Col("age")).filter(Col("age") > 1)
        .group_by(Col("country")).agg(F.count()), _edit(_first, lambda st: setattr(st.consumers[1], "condition", F.sum(Col("age")) > 1)))
    add("scan/too_many_numeric_columns", lambda t: _df(t["wide"]).group_by(Col("c00")).agg(*_sum_all([f"c{i:02d}" for i in range(1, 14)])))
    add("scan/many_sums_of_one_table", lambda t: _df(t["wide"]).group_by(Col("c00")).agg(*_sum_all([f"c{i:02d}" for i in range(1, 9)])))
    add("select/second_projection", lambda t: _df(t["users"]).select(Col("age"), Col("country")).select(Col("age")))
    add("select/writer_schema_differs", lambda t: _df(t["users"]),
        _edit(_first, lambda st: setattr(st.writer, "inferred_schema", st.writer.inferred_schema[:-1])))
    add("select/unknown_column", lambda t: _df(t["users"]).select(Col("age"), Col("country")), _edit(_first, _unknown_in_first_projection))
    add("select/string_expression", lambda t: _df(t["users"]).select(Col("first_name") + "!", Col("age")))
    add("select/many_computed_columns", lambda t: _df(t["wide"]).select(*[(Col(f"c{i:02d}") + i).alias(f"x{i}") for i in range(20)]))
    add("select/timestamp_difference", lambda t: _df(t["orders"]).select((Col("order_date") - Col("order_date")).alias("d"), Col("price")))
    add("select/comparison_as_a_column", lambda t: _df(t["orders"]).select((Col("price") > 3).alias("dear"), Col("price")))
    add("select/result_schema_mismatch", lambda t: _df(t["users"]).select(Col("age"), Col("country")),
        _edit(_first, lambda st: setattr(st.writer, "inferred_schema", st.writer.inferred_schema[:-1])))
    add("select/more_columns_than_a_result_holds", lambda t: _df(t["wide"]).select(*[Col(f"c{i:02d}") for i in range(40)]))
    add("select/numeric_where", lambda t: _df(t["users"]).filter(Col("age") > 30).filter(Col("country") == "USA").select(Col("age")),
        _edit(_first, lambda st: setattr(st.consumers[0], "condition", Col("age") - 30)))
    add("join_inputs/not_a_table_scan", lambda t: _df(t["users"]).group_by(Col("user_id")).agg(F.count())
        .join(_df(t["orders"]), on=Col("user_id") == Col("order_id"), how="inner").select(Col("product")))
    add("join_inputs/not_a_table_scan_group_by", lambda t: _df(t["users"]).group_by(Col("user_id")).agg(F.count())
        .join(_df(t["orders"]), on=Col("user_id") == Col("order_id"), how="inner").group_by(Col("product")).agg(F.count()))
    add("join_inputs/computed_column", lambda t: _df(t["users"]).select(Col("user_id"), (Col("age") * 2).alias("a2"))
        .join(_df(t["orders"]), on=Col("user_id") == Col("order_id"), how="inner").select(Col("product"), Col("a2")))
    add("join_inputs/aggregate_between", lambda t: _uo(t).select(Col("u.age")),
        _edit(_first, lambda st: st.consumers.append(AggregateTask(VoidTask(), group_by_column=Col("u.age"), agg_columns=[]))))
    add("join_inputs/key_is_projected_away", lambda t: _uo(t).select(Col("u.age")),
        _edit(_first, _prepend(_project(Col("u.age"), schema=[("u.age", T.INTEGER)]))))
    add("join_inputs/key_is_projected_away_group_by", lambda t: _uo(t).group_by(Col("u.country")).agg(F.count()),
        _edit(_first, _prepend(_project(Col("u.country"), schema=[("u.country", T.STRING)]))))
    add("join_inputs/unknown_name_in_a_where", lambda t: _uo(t).select(Col("u.age")), _edit(_first, _prepend(FilterTask(VoidTask(), condition=Col("nowhere") > 1))))
    add("join_inputs/aggregate_in_a_where", lambda t: _uo(t).select(Col("u.age")),
        _edit(_first, _prepend(FilterTask(VoidTask(), condition=F.sum(Col("u.age")) > 1))))
    add("join_rows/aggregate_after_the_join", lambda t: _uo(t).select(Col("u.age")),
        _edit(_join_stage, lambda st: st.consumers.append(AggregateTask(VoidTask(), group_by_column=Col("u.age"), agg_columns=[]))))
    add("join_rows/schema_mismatch", lambda t: _uo(t).select(Col("u.age"), Col("o.product")),
        _edit(_last, lambda st: setattr(st.writer, "inferred_schema", st.writer.inferred_schema[:-1])))
    add("join_rows/more_columns_than_a_result_holds", lambda t: _df(t["wide"]).join(_df(t["wide2"]), on=Col("c00") == Col("d00"), how="inner"))
    add("join_rows/where_over_many_columns", lambda t: _df(t["wide"]).join(_df(t["wide2"]), on=Col("c00") == Col("d00"), how="inner")
        .filter(_sum_of([f"c{i:02d}" for i in range(40)]) > 3).select(Col("c01")))
    add("join_rows/numeric_where", lambda t: _uo(t).filter(Col("o.quantity") > 1).select(Col("u.age")),
        _edit(_join_stage, lambda st: setattr(st.consumers[0], "condition", Col("o.quantity") - 1)))
    add("join_group/key_computed_after_the_join", lambda t: _bp(t).group_by(Col("bs")).agg(F.count()),
        _edit(_join_stage, lambda st: setattr(st.consumers[-1], "group_by_column", Col("bi") + 1)))
    add("join_group/filter_after_the_partial_aggregate", lambda t: _bp(t).group_by(Col("bs")).agg(F.count()),
        _edit(_join_stage, _append_filter(Col("count") > 1)))
    add("join_group/no_aggregate_pair", lambda t: _bp(t).group_by(Col("bs")).agg(F.count()), _edit(_last, _drop_consumers))
    add("byte_join/filter_between_table_and_join", lambda t: _df(t["jg_orders"]).filter(Col("o_totalprice") > 10)
        .join(_df(t["jg_lineitem"]), on=Col("o_orderkey") == Col("l_orderkey"), how="inner").group_by(Col("o_orderpriority")).agg(F.count()))
    add("byte_join/renamed_keys", lambda t: _df(t["jg_orders"]).select(Col("o_orderkey").alias("k"), Col("o_orderpriority"))
        .join(_df(t["jg_lineitem"]), on=Col("k") == Col("l_orderkey"), how="inner").group_by(Col("o_orderpriority")).agg(F.count()))
    add("byte_join/two_build_side_columns", lambda t: _jg(t).group_by(Col("o_orderpriority")).agg(F.sum(Col("o_totalprice")).alias("s")))
    add("byte_join/predicate_on_the_build_side", lambda t: _jg(t).filter(Col("o_orderpriority").like("1%")).group_by(Col("o_orderpriority"))
        .agg(F.count()))
    add("byte_join/numeric_build_side_column", lambda t: _jg(t).group_by(Col("l_orderkey")).agg(F.sum(Col("o_totalprice")).alias("s")))
    add("byte_join/probe_side_only", lambda t: _jg(t).filter(Col("l_quantity") > 10).group_by(Col("l_orderkey"))
        .agg(F.sum(Col("l_extendedprice")).alias("s"), F.avg(Col("l_quantity")).alias("a")))
    add("byte_join/many_probe_columns", lambda t: _df(t["names"]).join(_df(t["wide"]), on=Col("nk") == Col("c00"), how="inner")
        .group_by(Col("bs")).agg(*_sum_all([f"c{i:02d}" for i in range(1, 14)])))
    add("byte_join/eight_probe_columns", lambda t: _df(t["names"]).join(_df(t["wide"]), on=Col("nk") == Col("c00"), how="inner")
        .group_by(Col("bs")).agg(*_sum_all([f"c{i:02d}" for i in range(1, 9)])))
    add("byte_join/argument_reads_dictionary_codes", lambda t: _jg(t).group_by(Col("l_orderkey"))
        .agg(F.sum(Col("o_orderpriority").like("1%")).alias("urgent")))
    add("byte_join/input_is_not_a_scan", lambda t: _jg(t).group_by(Col("o_orderpriority")).agg(F.count()),
        _edit(_first, lambda st: setattr(st, "producer", VoidTask())))
    add("join_rows/input_is_not_a_scan", lambda t: _uo(t).select(Col("u.age")), _edit(_first, lambda st: setattr(st, "producer", VoidTask())))
    add("select/computed_column_stored_as_another_type", lambda t: _df(t["users"]).select((Col("age") + 1).alias("next"), Col("country")),
        _edit(_first, lambda st: setattr(st.writer, "inferred_schema", [("next", T.FLOAT), ("country", T.STRING)])))
    add("byte_join/dictionary_predicate",lambda t: _df(t["names"]).join(_df(t["p"]), on=Col("nk") == Col("pk"), how="inner")
        .filter(Col("ps").like("%e%")).group_by(Col("bs")).agg(F.count()))
    add("byte_join/filter_after_the_partial_aggregate", lambda t: _jg(t).group_by(Col("o_orderpriority")).agg(F.count()),
        _edit(_join_stage, _append_filter(Col("count") > 1)))
    add("byte_join/no_aggregate_pair", lambda t: _jg(t).group_by(Col("o_orderpriority")).agg(F.count()), _edit(_last, _drop_consumers))
    return out


def _sum_of(names: list[str]) -> Any:
    total = Col(names[0])
    for n in names[1:]:
        total = total + Col(n)
    return total


def _record(fn: str, task: Any, edit: Any) -> dict:
    """One call -> what a host has to reproduce: the blob's bytes (hashed), the tables, the result schema - or the refusal."""
    try:
        task = getattr(task, "task", task)
        blob, *paths, schema = getattr(stage, fn)(task, edit(task) if edit is not None else None)
    except Exception as exc:  # noqa: BLE001  (which exception, and its text, is what is pinned)
        return {"raises": type(exc).__name__, "message": re.sub(r"/[^\s'\"]*/", "", str(exc))}
    return {"sha256": hashlib.sha256(bytes(blob)).hexdigest(), "size": C.sizeof(blob), "paths": [Path(p).name for p in paths],
            "schema": [[n, t.name] for n, t in schema]}


def _records(tmp: Path) -> dict[str, dict]:
    tables = _tables(tmp)
    out = {}
    for name, build, edit in _cases():
        for fn in FUNCTIONS:
            try:
                task = build(tables)
            except Exception as exc:  # noqa: BLE001  (the frame itself is refused: the same for every function)
                out[f"{name}::{fn}"] = {"raises": type(exc).__name__, "message": f"(building the query) {exc}"}
                continue
            out[f"{name}::{fn}"] = _record(fn, task, edit)
    return out


def test_every_blob_and_every_refusal_is_the_recorded_one(tmp_path):
    want = json.loads(FIXTURE.read_text())
    got = _records(tmp_path)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} differ; the first: {next(iter(wrong.items()))}"


def test_the_corpus_lowers_through_every_function_and_no_result_name_keeps_a_dot(tmp_path):
    """At least three lowered cases per function; and the planner strips alias prefixes from the writer's schema
    (plan.py cleanup_output_column_names), so a result name never holds a dot when it reaches the blob."""
    got = _records(tmp_path)
    for fn in FUNCTIONS:
        assert sum(1 for k, r in got.items() if k.endswith(f"::{fn}") and "sha256" in r) >= 3, fn
    edited = {name for name, _, edit in _cases() if edit is not None}
    dotted = [k for k, r in got.items() if "sha256" in r and k.split("::")[0] not in edited and any("." in n for n, _ in r["schema"])]
    assert not dotted, dotted


def _raise_sites() -> dict[int, str]:
    lines = Path(stage.__file__).read_text().splitlines()
    return {i + 1: line.strip() for i, line in enumerate(lines) if re.search(r"raise (StageUnsupported|ValueError)\(", line)}


if __name__ == "__main__":
    import tempfile

    if "--write" not in sys.argv:
        sys.exit("usage: python -m tests.test_stage_plan_blobs --write   (on the commit whose behaviour is to be pinned)")
    sites, hit = _raise_sites(), set()

    def _trace(frame: Any, event: str, arg: Any) -> Any:
        if frame.f_code.co_filename != stage.__file__:
            return None
        if event == "line" and frame.f_lineno in sites:
            hit.add(frame.f_lineno)
        return _trace

    with tempfile.TemporaryDirectory() as tmp:
        sys.settrace(_trace)
        records = _records(Path(tmp))
        sys.settrace(None)
    FIXTURE.write_text(json.dumps(records, indent=0, sort_keys=True) + "\n")
    for fn in FUNCTIONS:
        mine = [r for k, r in records.items() if k.endswith(f"::{fn}")]
        print(f"{fn}: {sum('sha256' in r for r in mine)} lower, {sum('raises' in r for r in mine)} refuse")
    print(f"raise sites hit: {len(hit)} of {len(sites)}")
    for line in sorted(set(sites) - hit):
        print(f"  not reached: {line}: {sites[line]}")
