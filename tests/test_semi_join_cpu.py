"""LEFT SEMI / LEFT ANTI joins without a GPU: the four SQL spellings against the API call, where the right-side conjuncts
of the condition end up, the schema and the refusals of ``SemiJoinTask``, the plan's stages, the stage lowerings' refusal and
the argument checks and host-side geometry of hs_keyset_* / hs_mask_from_counts - and two guards that hold before the
feature too: the parser corpus recorded before SELECT DISTINCT keeps its trees, and an inner-join text renders as it did."""

from __future__ import annotations

import ctypes as C
import json
import re
from pathlib import Path

import pytest

from minispark_amd import hipspark as hs
from minispark_amd import tasks as t
from minispark_amd.constants import ColumnType as T
from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SqlSyntaxError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col, Functions as F
from tests.conftest import ROOT, load_golden
from tests.test_parser import render

CORPUS = json.loads((Path(__file__).parent / "golden" / "distinct_parser_corpus.json").read_text())
PATHS = load_golden("join_group")["paths"]
ORDERS, LINEITEM = PATHS["orders"], PATHS["lineitem"]
KEY = Col("o_orderkey") == Col("l_orderkey")


def table(path):
    return DataFrame(object()).table(path)


def tree(task):
    """tests.test_parser.render, with both inputs of a SemiJoinTask (render follows the left one only)."""
    lines, node = render(task), task
    for i in range(len(lines)):
        if type(node) is t.SemiJoinTask:
            lines[i] += " right=" + repr(tree(node.right_side_task))
        node = node.parent_task
    return lines


# ---- grammar ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling,how", [("SEMI JOIN", "left_semi"), ("LEFT SEMI JOIN", "left_semi"), ("ANTI JOIN", "left_anti"),
                                          ("LEFT ANTI JOIN", "left_anti")])
def test_each_spelling_builds_the_tree_of_the_api_call(spelling, how):
    sql = parse_sql(f"SELECT o_orderkey FROM 'orders' {spelling} 'lineitem' ON o_orderkey = l_orderkey;", object()).task
    api = table("orders").join(table("lineitem"), on=KEY, how=how).select(Col("o_orderkey")).task
    assert tree(sql) == tree(api)
    join = sql.parent_task
    assert type(join) is t.SemiJoinTask and join.anti == (how == "left_anti")
    assert join.describe() == f'SemiJoin((o_orderkey) == (l_orderkey), "{how}")'
    assert tree(sql)[1].endswith("right=['LoadTableBlockTask(lineitem) alias=']")


def test_aliases_and_a_where_around_a_semi_join():
    sql = parse_sql("SELECT o.o_orderkey FROM 'orders' AS o LEFT SEMI JOIN 'lineitem' AS l ON o.o_orderkey = l.l_orderkey "
                    "WHERE o.o_totalprice > 10;", object()).task
    api = (table("orders").alias("o").join(table("lineitem").alias("l"), on=Col("o.o_orderkey") == Col("l.l_orderkey"),
                                            how="left_semi")
           .filter(Col("o.o_totalprice") > 10).select(Col("o.o_orderkey")).task)
    assert tree(sql) == tree(api)


def test_joins_apply_left_to_right():
    sql = parse_sql("SELECT a FROM 'x' JOIN 'y' ON a = b LEFT ANTI JOIN 'z' ON a = c;", object()).task
    anti = sql.parent_task
    assert type(anti) is t.SemiJoinTask and anti.anti and type(anti.parent_task) is t.BroadcastHashJoinTask
    assert anti.parent_task.how == "inner"


def test_a_right_side_conjunct_goes_to_the_right_input():
    sql = parse_sql(f"SELECT o_orderkey FROM '{ORDERS}' LEFT SEMI JOIN '{LINEITEM}' ON o_orderkey = l_orderkey AND l_quantity > 45;",
                    object()).task
    join = sql.parent_task
    assert join.validate_schema() == table(ORDERS).schema
    assert (join.left_key.name, join.right_key.name) == ("o_orderkey", "l_orderkey")
    where = str(parse_sql("SELECT a FROM 't' WHERE l_quantity > 45;", object()).task.parent_task.condition)  # as the parser spells it
    assert [str(c) for c in join.right_filters] == [where]
    plan = PhysicalPlan.generate_physical_plan(sql)
    right = plan.stages[1]
    assert [type(c).__name__ for c in right.consumers] == ["FilterTask", "ProjectTask"]
    assert str(right.consumers[0].condition) == where
    assert [c.name for c in right.consumers[1].columns] == ["l_orderkey"]
    assert right.writer.inferred_schema == [("l_orderkey", T.INTEGER)]  # only the key column is materialised


@pytest.mark.parametrize("text", [
    "SELECT a FROM 'x' LEFT SEMI 'y' ON a = b;",
    "SELECT a FROM 'x' SEMI JOIN 'y';",
    "SELECT a FROM 'x' SEMI JOIN 'y' WHERE a = 1;",
    "SELECT a FROM 'x' ANTI SEMI JOIN 'y' ON a = b;",
    "SELECT a FROM 'x' LEFT SEMI ANTI JOIN 'y' ON a = b;",
    "SELECT a FROM 'x' SEMIJOIN 'y' ON a = b;",
])
def test_malformed_forms_are_syntax_errors(text):
    with pytest.raises(SqlSyntaxError):
        parse_sql(text, object())


@pytest.mark.parametrize("text", sorted(CORPUS), ids=[f"{i:02d}" for i in range(len(CORPUS))])
def test_a_text_accepted_before_builds_the_tree_it_built_before(text):
    assert render(parse_sql(text, object()).task) == CORPUS[text]


@pytest.mark.parametrize("kind", ["JOIN", "LEFT JOIN", "RIGHT JOIN", "INNER JOIN", "FULL JOIN"])
def test_an_inner_join_text_renders_as_it_did(kind):
    task = parse_sql(f"SELECT a FROM 'x' {kind} 'y' AS r ON a = r.b WHERE a > 1;", object()).task
    assert render(task) == ["Project(a)", "Filter((a gt 1))",
                            "Join((a) == (r.b), \"inner\") right=['LoadTableBlockTask(y) alias=r']",
                            "LoadTableBlockTask(x) alias="]
    assert type(task.parent_task.parent_task) is t.BroadcastHashJoinTask


def test_other_kinds_of_the_api_build_what_they_built():
    for how in ("inner", "left", "right", "outer"):
        task = table("x").join(table("y"), on=Col("a") == Col("b"), how=how).task
        assert type(task) is t.BroadcastHashJoinTask and task.how == how
    assert "SemiJoinTask" in t.__all__
    assert set(t.JoinType.__args__) == {"inner", "left", "right", "outer", "left_semi", "left_anti"}


# ---- schema and errors -----------------------------------------------------------------------------------------------------
def semi(on, how="left_semi", right=None):
    return table(ORDERS).join(right if right is not None else table(LINEITEM), on=on, how=how)


def test_the_result_schema_is_the_left_one():
    assert semi(KEY).schema == [("o_orderkey", T.INTEGER), ("o_orderpriority", T.STRING), ("o_totalprice", T.FLOAT)]
    assert semi(KEY, "left_anti").schema == table(ORDERS).schema
    assert semi(Col("l_orderkey") == Col("o_orderkey")).schema == table(ORDERS).schema  # either order of the equality


def test_a_right_column_after_the_join_is_an_unknown_column():
    with pytest.raises(ValueError, match=r"Unknown columns in projection: \['l_quantity'\]"):
        PhysicalPlan.generate_physical_plan(semi(KEY).select(Col("o_orderkey"), Col("l_quantity")).task)
    with pytest.raises(ValueError, match="Unknown columns"):
        PhysicalPlan.generate_physical_plan(
            parse_sql(f"SELECT o_orderkey, l_quantity FROM '{ORDERS}' SEMI JOIN '{LINEITEM}' ON o_orderkey = l_orderkey;", object()).task)


def test_float_and_mixed_keys_are_type_errors_that_name_both_columns():
    with pytest.raises(TypeError, match="o_totalprice.*l_quantity"):
        semi(Col("o_totalprice") == Col("l_quantity")).schema
    with pytest.raises(TypeError, match="o_orderkey.*l_shipmode"):
        semi(Col("o_orderkey") == Col("l_shipmode")).schema
    with pytest.raises(TypeError, match="o_orderpriority.*l_shipdate"):
        PhysicalPlan.generate_physical_plan(semi(Col("o_orderpriority") == Col("l_shipdate"), "left_anti").task)
    assert semi(Col("o_orderpriority") == Col("l_shipmode")).schema == table(ORDERS).schema  # STRING = STRING


def test_left_only_and_two_sided_conjuncts_are_value_errors_that_quote_them():
    left_only = Col("o_totalprice") > 100
    with pytest.raises(ValueError, match="WHERE") as e:
        semi(KEY & left_only).schema
    assert str(left_only) in str(e.value)
    two_sided = Col("o_totalprice") > Col("l_extendedprice")
    with pytest.raises(ValueError, match="both inputs") as e:
        semi(KEY & two_sided).schema
    assert str(two_sided) in str(e.value)
    with pytest.raises(ValueError, match="both inputs"):  # a second equality between the sides
        semi(KEY & (Col("o_orderpriority") == Col("l_shipmode"))).schema
    with pytest.raises(ValueError, match="Unknown columns in Join"):
        semi(KEY & (Col("nope") > 1)).schema


def test_a_key_that_is_no_equality_of_plain_columns_is_refused():
    for on in (Col("o_orderkey") < Col("l_orderkey"), (Col("o_orderkey") + 1) == Col("l_orderkey")):
        with pytest.raises(ValueError, match="both inputs") as e:
            semi(on).schema
        assert str(on) in str(e.value)
    with pytest.raises(ValueError, match="holds no equality"):
        semi(Col("l_quantity") > 45).schema


# ---- plan ------------------------------------------------------------------------------------------------------------------
def test_the_stages_of_a_semi_join(capsys):
    df = semi(KEY & (Col("l_quantity") > 45)).group_by(Col("o_orderpriority")).agg(F.count().alias("n"))
    plan = PhysicalPlan.generate_physical_plan(df.task)
    assert [repr(s) for s in plan.stages] == [
        "[Stage 0: LoadTableBlockTask -> WriteToShufflePartitions, deps: ()]",
        "[Stage 1: LoadTableBlockTask -> [FilterTask,ProjectTask] -> WriteToShufflePartitions, deps: ()]",
        "[Stage 2: SemiJoinTask -> [AggregateTask] -> WriteToShufflePartitions, deps: (0,1)]",
        "[Stage 3: LoadShuffleFilesTask -> [AggregateTask] -> WriteToLocalFileTask, deps: (2)]"]
    assert plan.stages[2].producer.inferred_schema == table(ORDERS).schema
    assert df.task.parent_task.expanded is False  # the caller's tree is planned on a copy
    df.explain()
    shown = capsys.readouterr().out
    assert 'SemiJoin(((o_orderkey) == (l_orderkey)) and ((l_quantity) > (45)), "left_semi")' in shown
    assert f"LoadTableBlockTask({ORDERS})" in shown and f"LoadTableBlockTask({LINEITEM})" in shown  # both inputs


def test_a_plain_semi_join_writes_the_left_columns():
    plan = PhysicalPlan.generate_physical_plan(semi(KEY, "left_anti").task)
    assert [type(s.producer).__name__ for s in plan.stages] == ["LoadTableBlockTask", "LoadTableBlockTask", "SemiJoinTask"]
    assert plan.stages[2].writer.inferred_schema == table(ORDERS).schema and plan.stages[2].consumers == []
    assert [c.name for c in plan.stages[1].consumers[0].columns] == ["l_orderkey"]


def test_a_sort_under_the_right_side_is_refused():
    with pytest.raises(ValueError, match="must be the last operation"):
        PhysicalPlan.generate_physical_plan(semi(KEY, right=table(LINEITEM).order_by(Col("l_orderkey")).limit(5)).task)
    with pytest.raises(ValueError, match="must be the last operation"):
        PhysicalPlan.generate_physical_plan(table(ORDERS).limit(5).join(table(LINEITEM), on=KEY, how="left_semi").task)


def test_all_five_stage_lowerings_refuse_a_semi_join():
    from minispark_amd import stage

    lowerings = [stage.lower_stage_plan, stage.lower_join_stage_plan, stage.lower_select_stage_plan,
                 stage.lower_join_select_stage_plan, stage.lower_join_group_stage_plan]
    queries = [semi(KEY), semi(KEY, "left_anti").select(Col("o_orderkey")),
               semi(KEY).group_by(Col("o_orderpriority")).agg(F.count().alias("n"), F.sum(Col("o_totalprice")).alias("s"))]
    for lower in lowerings:
        for df in queries:
            with pytest.raises(stage.StageUnsupported):
                lower(df.task)


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------
def _constants():
    text = (ROOT / "minispark_amd" / "csrc" / "hs_radix.hip").read_text()
    env: dict[str, int] = {}
    for m in re.finditer(r"constexpr int (KS_\w+) = ([^;]+);", text):
        env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))  # noqa: S307 - the repository's own source
    return env


def test_keyset_arguments_are_checked_without_a_gpu():
    lib = hs.load_library()
    one = C.c_void_p(4096)  # a non-null, aligned address: every call below is refused before anything is touched
    bad_builds = [dict(keys=None), dict(bitmap=None), dict(ws=None), dict(flags=None), dict(slots=0), dict(slots=(1 << 32) + 1),
                  dict(n=1 << 31), dict(n=-1), dict(bitmap=C.c_void_p(4100)), dict(key_min=5, slots=1 << 32)]
    for bad in bad_builds:
        a = dict(keys=one, n=10, key_min=0, slots=100, bitmap=one, ws=one, flags=one) | bad
        rc = lib.hs_keyset_build(None, a["keys"], a["n"], a["key_min"], a["slots"], a["bitmap"], a["ws"], a["flags"])
        assert rc == 1 and b"hs_keyset_build: bad arguments" in lib.hs_last_error(), bad
    bad_probes = [dict(keys=None), dict(bitmap=None), dict(mask=None), dict(slots=0), dict(slots=(1 << 32) + 1), dict(n=1 << 31),
                  dict(n=-1), dict(keys=C.c_void_p(4100)), dict(mask=C.c_void_p(4097))]
    for bad in bad_probes:
        a = dict(keys=one, n=10, key_min=0, slots=100, bitmap=one, anti=0, mask=one) | bad
        rc = lib.hs_keyset_probe(None, a["keys"], a["n"], a["key_min"], a["slots"], a["bitmap"], a["anti"], a["mask"])
        assert rc == 1 and b"hs_keyset_probe: bad arguments" in lib.hs_last_error(), bad
    for counts, n, mask in [(None, 4, one), (one, 4, None), (one, -1, one), (C.c_void_p(4104), 4, one), (one, 4, C.c_void_p(4098))]:
        assert lib.hs_mask_from_counts(None, counts, n, 0, mask) == 1
        assert b"hs_mask_from_counts: bad arguments" in lib.hs_last_error()
    # empty probes are no launch
    assert lib.hs_keyset_probe(None, None, 0, 0, 1, one, 0, None) == 0 and lib.hs_mask_from_counts(None, None, 0, 1, None) == 0


def test_keyset_geometry_without_a_gpu():
    lib = hs.load_library()
    k = _constants()
    L = k["KS_L"]
    assert 16 <= L <= 19 and k["KS_CHUNK"] >= 1024
    slack = k["KS_SLACK"]
    assert lib.hs_keyset_bitmap_bytes(0) == 0 and lib.hs_keyset_bitmap_bytes(-1) == 0 and lib.hs_keyset_bitmap_bytes((1 << 32) + 1) == 0
    for slots, words in [(1, 1), (32, 1), (33, 2), (128, 4), (129, 5), ((1 << L) + 1, (1 << (L - 5)) + 1), (1 << 32, 1 << 27)]:
        nbytes = lib.hs_keyset_bitmap_bytes(slots)
        assert nbytes == (words + 3) // 4 * 16 + slack and nbytes >= 4 * words, slots  # whole 16-byte groups + the slack
    assert lib.hs_keyset_bitmap_bytes(33) >= 8  # two words
    # no pass (one partition), one pass, two passes: each a workspace; two passes hold two copies of the keys, one pass one
    n = 1_000_000
    none, one, two = (lib.hs_keyset_ws_bytes(n, s) for s in (1 << L, 1 << (L + 8), 1 << (L + 9)))
    assert 0 < none < 4 * n < one < 8 * n < two < 12 * n
    assert 4 * n < lib.hs_keyset_ws_bytes(n, (1 << L) + 1) <= one and lib.hs_keyset_ws_bytes(0, 1) > 0
    assert lib.hs_keyset_ws_bytes(n, 1 << 32) > 0
    assert lib.hs_keyset_ws_bytes(n, 0) == 0 and lib.hs_keyset_ws_bytes(n, (1 << 32) + 1) == 0
    assert lib.hs_keyset_ws_bytes(1 << 31, 100) == 0 and lib.hs_keyset_ws_bytes(-1, 100) == 0
    # the keys alone travel: half of what the dense join's (key, row) tuples take over the same range
    assert lib.hs_keyset_ws_bytes(n, 1 << 26) < lib.hs_join_dense_ws_bytes(n, 1 << 26) * 0.6
