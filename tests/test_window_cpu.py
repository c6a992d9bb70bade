"""Window ranking without a GPU: the numpy definition on hand-written cases, the grammar against the API, where window
items may stand, the refusals of the API, the parser, the planner and the stage lowerings, the argument checks of
hs_window - and the guard that a plain SortTask prints as it did."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from minispark_amd import tasks as t
from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SemanticError, SqlSyntaxError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col, Lit, WindowItem
from minispark_amd.sql import Functions as F
from tests.conftest import load_golden
from tests.test_distinct_cpu import _golden_frames
from tests.test_parser import render
from tests.window_model import codes, window_model


def T(name="t"):
    return DataFrame(object()).table(name)


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_the_model_on_ties_in_input_order():
    part = ["a", "b", "a", "a", "b", "a"]
    value = [5, 1, 5, 3, 1, 9]
    got = window_model(6, [part], [(value, True)])
    assert got["row_number"].tolist() == [2, 1, 3, 1, 2, 4]  # the two 5s of 'a': the earlier row first
    assert got["rank"].tolist() == [2, 1, 2, 1, 1, 4]
    assert got["dense_rank"].tolist() == [2, 1, 2, 1, 1, 3]


def test_the_model_descending_and_without_keys():
    value = [5, 1, 5, 3]
    got = window_model(4, [], [(value, False)])
    assert got["row_number"].tolist() == [1, 4, 2, 3] and got["rank"].tolist() == [1, 4, 1, 3]
    assert got["dense_rank"].tolist() == [1, 3, 1, 2]
    got = window_model(4, [[7, 8, 7, 8]], [])
    assert got["row_number"].tolist() == [1, 1, 2, 2] and got["rank"].tolist() == [1, 1, 1, 1]
    assert window_model(0, [[]], [([], True)])["rank"].tolist() == []


def test_the_model_orders_nan_last_and_takes_both_zeros_as_one_value():
    nan = float("nan")
    value = [nan, -0.0, float("inf"), 0.0, float("-inf"), nan, 1.5]
    assert codes(value).tolist()[1] == codes(value).tolist()[3] and codes(value)[0] == codes(value)[5]
    got = window_model(7, [], [(value, True)])
    assert got["rank"].tolist() == [6, 2, 5, 2, 1, 6, 4] and got["dense_rank"].tolist() == [5, 2, 4, 2, 1, 5, 3]
    assert got["row_number"].tolist() == [6, 2, 5, 3, 1, 7, 4]
    got = window_model(7, [value], [])  # as a partition column: -0.0 and 0.0 share a partition, the NaNs another
    assert got["row_number"].tolist() == [1, 1, 1, 2, 1, 2, 1]


def test_the_model_compares_strings_by_bytes_and_length():
    value = [b"ab\0", b"ab", b"b", b"", b"ab"]
    assert window_model(5, [], [(value, True)])["rank"].tolist() == [4, 2, 5, 1, 2]


# ---- grammar and API ---------------------------------------------------------------------------------------------------
CASES = [
    ("SELECT a, b, ROW_NUMBER() OVER (PARTITION BY a ORDER BY b DESC) AS rn FROM 't';",
     lambda: T().select(Col("a"), Col("b")).window(F.row_number().over(partition_by=[Col("a")], order_by=[Col("b").desc()]).alias("rn"))),
    ("SELECT a, RANK() OVER (ORDER BY a) FROM 't' ORDER BY rank LIMIT 3;",
     lambda: T().select(Col("a")).window(F.rank().over(order_by=[Col("a")])).order_by(Col("rank")).limit(3)),
    ("SELECT a, b, DENSE_RANK()  OVER( PARTITION BY a, b  ORDER BY a ASC, b DESC ) AS d FROM 't' WHERE a > 1 QUALIFY d <= 3;",
     lambda: T().filter(Col("a") > Lit(1)).select(Col("a"), Col("b"))
     .window(F.dense_rank().over(partition_by=[Col("a"), Col("b")], order_by=[Col("a").asc(), Col("b").desc()]).alias("d"))
     .qualify(Col("d") <= Lit(3))),
    ("SELECT DISTINCT a, ROW_NUMBER() OVER () AS rn FROM 't' QUALIFY rn > 1 ORDER BY rn DESC LIMIT 2;",
     lambda: T().select(Col("a")).window(F.row_number().over().alias("rn")).qualify(Col("rn") > Lit(1)).distinct()
     .order_by(Col("rn").desc()).limit(2)),
    ("SELECT ROW_NUMBER() OVER (ORDER BY a) AS rn, a, RANK() OVER (ORDER BY a) AS rk, b FROM 't';",
     lambda: T().select(Col("a"), Col("b")).window(F.row_number().over(order_by=[Col("a")]).alias("rn"),
                                                   F.rank().over(order_by=[Col("a")]).alias("rk"),
                                                   select_order=["rn", "a", "rk", "b"])),
    ("SELECT k, COUNT() AS n, RANK() OVER (ORDER BY n DESC) AS r FROM 't' GROUP BY k HAVING n > 1 QUALIFY r <= 2 ORDER BY r;",
     lambda: T().group_by(Col("k")).agg(F.count().alias("n")).filter(Col("n") > Lit(1)).select(Col("k"), Col("n"))
     .window(F.rank().over(order_by=[Col("n").desc()]).alias("r")).qualify(Col("r") <= Lit(2)).order_by(Col("r"))),
]


@pytest.mark.parametrize("sql,build", CASES, ids=[f"{i}" for i in range(len(CASES))])
def test_text_builds_the_same_tree_as_the_api(sql, build):
    got, want = parse_sql(sql, object()).task, build().task
    assert type(got) is t.SortTask and got.windows and type(got.parent_task) is not t.SortTask  # ONE task carries all
    assert render(got) == render(want) and repr(got) == repr(want)
    assert got.validate_schema() == want.validate_schema() if "'t'" not in sql else True


def test_window_items_stand_anywhere_and_the_result_has_select_list_order():
    g = load_golden("e2e_join_select")
    orders = g["paths"]["orders"]
    text = (f"SELECT ROW_NUMBER() OVER (ORDER BY price) AS first, product, RANK() OVER (PARTITION BY product ORDER BY quantity DESC), "
            f"quantity, price, DENSE_RANK() OVER (ORDER BY product) AS last FROM '{orders}';")
    task = parse_sql(text, object()).task
    names = [name for name, _ in task.validate_schema()]
    assert names == ["first", "product", "rank", "quantity", "price", "last"]
    assert [str(ty) for _, ty in task.validate_schema()].count("INTEGER") >= 4
    assert [c.name for c in task.parent_task.columns] == ["product", "quantity", "price"]  # the items were set aside
    trailing = parse_sql(f"SELECT *, ROW_NUMBER() OVER (ORDER BY price) AS rn FROM '{orders}';", object()).task
    assert trailing.select_order is None and trailing.validate_schema()[-1][0] == "rn"
    with pytest.raises(SemanticError, match="come last"):
        parse_sql(f"SELECT ROW_NUMBER() OVER (ORDER BY price) AS rn, * FROM '{orders}';", object())
    appended = T(orders).select(Col("product")).window(F.row_number().over().alias("x"), F.row_number().over().alias("y"))
    assert [name for name, _ in appended.task.validate_schema()] == ["product", "x", "y"]


def test_window_items_with_group_by_name_the_grouped_columns():
    orders = load_golden("e2e_join_select")["paths"]["orders"]
    text = (f"SELECT product, RANK() OVER (ORDER BY top DESC) AS r, MAX(price) AS top FROM '{orders}' "
            "GROUP BY product QUALIFY r = 1;")
    task = parse_sql(text, object()).task
    assert [name for name, _ in task.validate_schema()] == ["product", "r", "top"]
    assert render(task)[1:] == render(parse_sql(f"SELECT product, MAX(price) AS top FROM '{orders}' GROUP BY product;", object()).task)
    plan = PhysicalPlan.generate_physical_plan(task)
    assert [name for name, _ in plan.stages[-1].writer.inferred_schema] == ["product", "r", "top"]
    with pytest.raises(ValueError, match="quantity"):   # not a column of the grouped result
        parse_sql(f"SELECT product, RANK() OVER (ORDER BY quantity) AS r FROM '{orders}' GROUP BY product;",
                  object()).task.validate_schema()


def test_describe_names_the_items():
    task = parse_sql("SELECT a, RANK() OVER (PARTITION BY a ORDER BY b DESC) AS r, b FROM 't' QUALIFY r < 3 LIMIT 9;", object()).task
    assert task.describe() == "Window(RANK() OVER (PARTITION BY a ORDER BY b DESC) AS r; QUALIFY (3) > (r)) -> Sort(; limit=9)"
    assert "windows=[RANK() OVER (PARTITION BY a ORDER BY b DESC) AS r]" in repr(task) and "select_order=['a', 'r', 'b']" in repr(task)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_rank_and_dense_rank_need_an_order_by():
    for text in ("SELECT a, RANK() OVER (PARTITION BY a) FROM 't';", "SELECT a, DENSE_RANK() OVER () FROM 't';"):
        with pytest.raises(ValueError, match="needs an ORDER BY inside OVER"):
            parse_sql(text, object())
    with pytest.raises(ValueError, match="needs an ORDER BY inside OVER"):
        F.rank().over(partition_by=[Col("a")])
    assert parse_sql("SELECT a, ROW_NUMBER() OVER (PARTITION BY a) FROM 't';", object()).task.windows[0].order_by == []
    with pytest.raises(ValueError, match="over"):
        T().select(Col("a")).window(F.row_number())  # no .over(...)


def test_qualify_without_a_window_item():
    with pytest.raises(SemanticError, match="QUALIFY.*no window item"):
        parse_sql("SELECT a FROM 't' QUALIFY a > 1;", object())
    with pytest.raises(ValueError, match="follows window"):
        T().select(Col("a")).qualify(Col("a") > 1)
    with pytest.raises(ValueError, match="no window item"):
        t.SortTask(_golden_frames()["scan"]().task, qualify=Col("quantity") > 1).validate_schema()


def test_an_expression_or_another_window_item_is_no_key():
    with pytest.raises(ValueError, match="plain columns"):
        F.row_number().over(order_by=[Col("a") + 1])
    with pytest.raises(ValueError, match="plain columns"):
        F.rank().over(partition_by=[Col("a") * 2], order_by=[Col("a")])
    with pytest.raises(SemanticError, match="Unsupported function"):  # no window item: the function call it was before
        parse_sql("SELECT a, ROW_NUMBER() OVER (ORDER BY a + 1) FROM 't';", object())
    with pytest.raises(SqlSyntaxError):
        parse_sql("SELECT a, ROW_NUMBER() OVER (ORDER BY a) AS rn FROM 't' QUALIFY;", object())
    orders = load_golden("e2e_join_select")["paths"]["orders"]
    two = T(orders).select(Col("product")).window(F.row_number().over(order_by=[Col("product")]).alias("rn"),
                                                  F.rank().over(order_by=[Col("rn")]).alias("rk"))
    with pytest.raises(ValueError, match='"rn" not found'):
        two.task.validate_schema()
    twice = T(orders).select(Col("product")).window(F.row_number().over(), F.row_number().over(order_by=[Col("product")]))
    with pytest.raises(ValueError, match="Duplicate.*row_number"):
        twice.task.validate_schema()


def test_a_ninth_item_and_a_thirteenth_key_name_their_limits():
    items = [F.row_number().over(order_by=[Col("a")]).alias(f"w{i}") for i in range(9)]
    with pytest.raises(ValueError, match="at most 8 window items"):
        T().select(Col("a")).window(*items)
    assert len(T().select(Col("a")).window(*items[:8]).task.windows) == 8
    text = "SELECT a, " + ", ".join(f"ROW_NUMBER() OVER (ORDER BY a) AS w{i}" for i in range(9)) + " FROM 't';"
    with pytest.raises(ValueError, match="at most 8 window items"):
        parse_sql(text, object())
    with pytest.raises(ValueError, match="at most 12"):
        T().select(Col("a")).window(F.row_number().over(partition_by=[Col("a")] * 7, order_by=[Col("a")] * 6))


def test_window_comes_before_qualify_distinct_order_by_and_limit():
    item = lambda: F.row_number().over(order_by=[Col("a")]).alias("rn")  # noqa: E731
    for early in (lambda df: df.order_by(Col("a")), lambda df: df.limit(3), lambda df: df.distinct()):
        with pytest.raises(ValueError, match="before"):
            early(T().select(Col("a"))).window(item())
    with pytest.raises(ValueError, match="once"):
        T().select(Col("a")).window(item()).window(item())
    with pytest.raises(ValueError, match="directly after window"):
        T().select(Col("a")).window(item()).distinct().qualify(Col("rn") > 1)
    with pytest.raises(ValueError, match="before limit"):
        T().select(Col("a")).window(item()).limit(2).order_by(Col("rn"))
    df = T().select(Col("a")).window(item())
    top = df.task
    df.qualify(Col("rn") > 1).distinct().order_by(Col("rn")).limit(4)
    assert df.task is top and top.distinct and top.limit == 4 and [str(c) for c, _ in top.keys] == ["rn"]


def test_a_window_below_a_join_or_another_operation_is_refused_when_planned():
    g = load_golden("e2e_join_select")
    right = (DataFrame(object()).table(g["paths"]["orders"]).alias("o")
             .window(F.row_number().over(order_by=[Col("o.price")]).alias("rn")))
    joined = DataFrame(object()).table(g["paths"]["users"]).alias("u").join(right, on=Col("u.user_id") == Col("o.user_id"),
                                                                            how="inner")
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(joined.task)
    below = _golden_frames()["scan"]().window(F.row_number().over(order_by=[Col("product")])).filter(Col("quantity") > 1)
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(below.task)


@pytest.mark.parametrize("text", ["SELECT a, ROW_NUMBER() AS rn FROM 't';", "SELECT ROW_NUMBER() FROM 't';",
                                  "SELECT a, RANK(a) OVER (ORDER BY a) FROM 't';", "SELECT DENSE_RANK(1) FROM 't';"])
def test_without_over_or_with_an_argument_it_is_the_unsupported_function_it_was(text):
    with pytest.raises(SemanticError, match="Unsupported function"):
        parse_sql(text, object())


# ---- planner and stage lowerings ---------------------------------------------------------------------------------------
KEYS = {"scan": "product", "group": "p", "join": "u.first_name", "join_group": "n"}


def ranked(shape):
    return _golden_frames()[shape]().window(F.rank().over(order_by=[Col(KEYS[shape])]).alias("r")).qualify(Col("r") < 4)


@pytest.mark.parametrize("shape", ["scan", "group", "join"])
def test_the_windowed_task_stays_in_the_result_stage_and_adds_its_columns(shape):
    plan = PhysicalPlan.generate_physical_plan(ranked(shape).task)
    for stage in plan.stages[:-1]:
        assert not any(type(x).__name__ == "SortTask" for x in stage.consumers)
    last = plan.stages[-1]
    assert type(last.writer).__name__ == "WriteToLocalFileTask"
    kinds = [type(x).__name__ for x in last.consumers]
    assert kinds.count("SortTask") == 1
    assert kinds[kinds.index("SortTask") + 1:] == (["ProjectTask"] if shape == "join" else [])
    sort = last.consumers[kinds.index("SortTask")]
    assert sort.inferred_schema == [*sort.input_schema, ("r", sort.inferred_schema[-1][1])]
    assert str(sort.inferred_schema[-1][1]) == "INTEGER" and last.writer.inferred_schema[-1] == sort.inferred_schema[-1]
    assert "." not in "".join(name for name, _ in last.writer.inferred_schema)  # the rename above carries the new column


def test_all_five_stage_lowerings_refuse_a_windowed_plan():
    from minispark_amd import stage as st

    lowerings = [st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                 st.lower_join_group_stage_plan]
    for lower in lowerings:
        for shape in KEYS:
            with pytest.raises(st.StageUnsupported):
                lower(ranked(shape).task)


def test_a_plain_sort_task_prints_as_before():
    task = t.SortTask(t.VoidTask(), keys=[(Col("a"), False)], limit=3)
    assert repr(task) == "SortTask(inferred_schema=None, keys=[(a, False)], limit=3)"
    assert task.describe() == "Sort(a DESC; limit=3)"
    assert repr(T().select(Col("a")).distinct().task).endswith("keys=[], limit=None, distinct=True)")
    assert isinstance(F.row_number(), WindowItem) and F.dense_rank().over(order_by=[Col("a")]).name == "dense_rank"


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu():
    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    key = (hs.hs_col * 13)()
    for k in range(13):
        key[k].kind, key[k].fixed_len, key[k].data = hs.I32, -1, 4096  # never dereferenced by the checks
    desc = (C.c_int32 * 13)()
    out = (C.c_void_p * 9)(*[4096] * 9)
    ws = (C.c_uint8 * 64)()

    def call(n_part=1, n_keys=2, nrows=4, funcs=(hs.WIN_ROW_NUMBER,), outs=out, work=ws, keys=key):
        kinds = (C.c_int32 * max(len(funcs), 1))(*funcs)
        return lib.hs_window(None, keys, desc, n_part, n_keys, nrows, kinds, len(funcs), outs, work, None)

    assert call(n_keys=13) == 2 and b"12" in lib.hs_last_error()
    assert call(nrows=1 << 31) == 2 and b"2^31" in lib.hs_last_error()
    assert call(funcs=[hs.WIN_ROW_NUMBER] * 9) == 2 and b"8" in lib.hs_last_error()
    assert call(n_part=2, funcs=(hs.WIN_ROW_NUMBER, hs.WIN_RANK)) == 1 and b"order key" in lib.hs_last_error()
    assert call(n_part=2, funcs=(hs.WIN_DENSE_RANK,)) == 1
    assert call(n_part=3) == 1 and call(n_part=-1) == 1 and call(nrows=-1) == 1 and call(funcs=()) == 1 and call(funcs=(3,)) == 1
    assert call(outs=None) == 1 and call(work=None) == 1 and call(keys=None) == 1
    assert call(nrows=0) == 0 and call(nrows=0, n_part=2) == 0  # nothing to number: nothing is launched
    assert lib.hs_window_ws_bytes(1 << 20, 2, 3) >= lib.hs_order_by_ws_bytes(1 << 20, 2, 3) + (1 << 20)
    assert (hs.WIN_ROW_NUMBER, hs.WIN_RANK, hs.WIN_DENSE_RANK, hs.WIN_MAX_FUNCS) == (0, 1, 2, 8)
    assert codes(np.arange(3)).tolist() == [0, 1, 2]
