"""ORDER BY / LIMIT without a GPU: the grammar against the API, the API's and the planner's refusals, where the
SortTask lands in the physical plan, the stage lowerings' refusal and the argument checks of hs_order_by."""

from __future__ import annotations

import ctypes as C

import pytest

from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SqlSyntaxError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col, Functions as F, Lit
from tests.conftest import load_golden
from tests.queries import api_namespace, case_by_name
from tests.sql_texts import E2E_SQL
from tests.test_parser import render


def T(name="t"):
    return DataFrame(object()).table(name)


CASES = [
    ("SELECT a, b FROM 't' ORDER BY a;", lambda: T().select(Col("a"), Col("b")).order_by(Col("a"))),
    ("SELECT a, b FROM 't' WHERE b > 2 ORDER BY a DESC, b ASC LIMIT 5;",
     lambda: T().filter(Col("b") > Lit(2)).select(Col("a"), Col("b")).order_by(Col("a").desc(), Col("b").asc()).limit(5)),
    ("SELECT k, COUNT() AS n FROM 't' GROUP BY k HAVING COUNT() > 1 ORDER BY n DESC LIMIT 3;",
     lambda: T().group_by(Col("k")).agg(F.count().alias("n"), F.count().alias("_having_count"))
     .filter(Col("_having_count") > Lit(1)).select(Col("k"), Col("n")).order_by(Col("n").desc()).limit(3)),
    ("SELECT a FROM 't' LIMIT 0;", lambda: T().select(Col("a")).limit(0)),
    ("SELECT a , b FROM 't' ORDER BY a ,b  DESC  LIMIT 12 ;",
     lambda: T().select(Col("a"), Col("b")).order_by(Col("a"), Col("b").desc()).limit(12)),
]


@pytest.mark.parametrize("sql,build", CASES, ids=[c[0][:50] for c in CASES])
def test_text_builds_the_same_tree_as_the_api(sql, build):
    got = render(parse_sql(sql, object()).task)
    assert got == render(build().task)
    assert got[0].startswith("Sort(")


def test_describe_names_keys_directions_and_limit(capsys):
    df = T().select(Col("k1"), Col("k2")).order_by(Col("k1"), Col("k2").desc()).limit(7)
    assert df.task.describe() == "Sort(k1 ASC, k2 DESC; limit=7)"
    assert T().select(Col("a")).order_by(Col("a")).task.describe() == "Sort(a ASC; limit=None)"


@pytest.mark.parametrize("tail", ["ORDER a", "ORDER BY", "LIMIT -1", "LIMIT 1.5", "LIMIT x", "ORDER BY a LIMIT 5 WHERE a > 1",
                                  "LIMIT 5 ORDER BY a", "ORDER BY a,", "ORDER BY a DESC ASC", "ORDERBY a"])
def test_malformed_clauses_are_syntax_errors(tail):
    with pytest.raises(SqlSyntaxError):
        parse_sql(f"SELECT a FROM 't' {tail};", object())


def test_order_by_takes_names_of_the_select_list():
    with pytest.raises(ValueError, match='"b"') as info:
        parse_sql("SELECT a FROM 't' ORDER BY b;", object())
    assert not isinstance(info.value, SqlSyntaxError)
    parse_sql("SELECT a + 1 AS b FROM 't' ORDER BY b;", object())  # an alias is a result name
    parse_sql("SELECT * FROM 't' ORDER BY b;", object())           # `*`: the schema decides, when the query is planned


@pytest.mark.parametrize("name", sorted(E2E_SQL))
def test_the_reference_texts_still_build_their_trees(name):
    assert len(E2E_SQL) == 20
    case = case_by_name(name)
    paths = {"users": "/data/users.bin", "orders": "/data/orders.bin"}
    api = api_namespace(lambda: DataFrame(object()), Col, F, Lit)
    tree = render(parse_sql(E2E_SQL[name].format(**paths), object()).task)
    assert tree == render(case.build(api, paths).task)
    assert not any(line.startswith("Sort(") for line in tree)


# ---- API and planner -------------------------------------------------------------------------------------------------
def test_api_refusals():
    with pytest.raises(ValueError, match="plain columns"):
        T().order_by(Col("a") + 1)
    with pytest.raises(ValueError, match="plain columns"):
        T().order_by((Col("a") * 2).desc())
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="LIMIT"):
            T().limit(bad)
        with pytest.raises(ValueError, match="LIMIT"):
            T().order_by(Col("a")).limit(bad)


def test_limit_after_order_by_is_one_task():
    df = T().select(Col("a")).order_by(Col("a").desc())
    sort = df.task
    df.limit(4)
    assert df.task is sort and sort.limit == 4 and [(str(c), asc) for c, asc in sort.keys] == [("a", False)]
    alone = T().select(Col("a")).limit(2)
    assert type(alone.task).__name__ == "SortTask" and alone.task.keys == [] and alone.task.limit == 2
    assert type(alone.task.parent_task).__name__ == "ProjectTask"


def _golden_frames():
    g = load_golden("e2e_join_select")
    users, orders = g["paths"]["users"], g["paths"]["orders"]
    scan = lambda: DataFrame(object()).table(orders).filter(Col("price") > 10).select(Col("product"), Col("quantity"))  # noqa: E731
    group = lambda: (DataFrame(object()).table(orders).group_by(Col("user_id")).agg(F.avg(Col("price")).alias("p"))  # noqa: E731
                     .select(Col("user_id"), Col("p")))
    join = lambda: (DataFrame(object()).table(users).alias("u")  # noqa: E731
                    .join(DataFrame(object()).table(orders).alias("o"), on=Col("u.user_id") == Col("o.user_id"), how="inner")
                    .select(Col("u.first_name"), Col("o.product")))
    return {"scan": (scan, "product"), "group": (group, "p"), "join": (join, "u.first_name")}


@pytest.mark.parametrize("shape", ["scan", "group", "join"])
def test_the_sort_task_sits_in_the_last_stage(shape):
    build, key = _golden_frames()[shape]
    plan = PhysicalPlan.generate_physical_plan(build().order_by(Col(key).desc()).limit(3).task)
    for stage in plan.stages[:-1]:
        assert not any(type(t).__name__ == "SortTask" for t in stage.consumers)
    last = plan.stages[-1]
    assert type(last.writer).__name__ == "WriteToLocalFileTask"
    kinds = [type(t).__name__ for t in last.consumers]
    assert kinds.count("SortTask") == 1
    after = kinds[kinds.index("SortTask") + 1:]
    assert after == (["ProjectTask"] if shape == "join" else [])  # only the planner's own renaming may follow it
    sort = last.consumers[kinds.index("SortTask")]
    assert sort.inferred_schema == sort.parent_task.inferred_schema


def test_unknown_key_and_misplaced_sort_are_refused_when_planned():
    build, _ = _golden_frames()["scan"]
    with pytest.raises(ValueError, match='Column "nope" not found in schema'):
        PhysicalPlan.generate_physical_plan(build().order_by(Col("nope")).task)
    with pytest.raises(ValueError, match="ORDER BY / LIMIT must be the last operation"):
        PhysicalPlan.generate_physical_plan(build().order_by(Col("product")).filter(Col("quantity") > 1).task)
    with pytest.raises(ValueError, match="ORDER BY / LIMIT must be the last operation"):
        PhysicalPlan.generate_physical_plan(build().limit(3).select(Col("product")).task)
    g = load_golden("e2e_join_select")
    right = DataFrame(object()).table(g["paths"]["orders"]).alias("o").limit(2)
    joined = DataFrame(object()).table(g["paths"]["users"]).alias("u").join(right, on=Col("u.user_id") == Col("o.user_id"),
                                                                            how="inner")
    with pytest.raises(ValueError, match="ORDER BY / LIMIT must be the last operation"):
        PhysicalPlan.generate_physical_plan(joined.task)


def test_all_five_stage_lowerings_refuse_a_sorted_plan():
    from minispark_amd import stage as st

    lowerings = [st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                 st.lower_join_group_stage_plan]
    frames = _golden_frames()
    g = load_golden("e2e_join_select")
    join_group = (DataFrame(object()).table(g["paths"]["users"]).alias("u")
                  .join(DataFrame(object()).table(g["paths"]["orders"]).alias("o"), on=Col("u.user_id") == Col("o.user_id"),
                        how="inner").group_by(Col("u.country")).agg(F.count().alias("n")).select(Col("u.country"), Col("n")))
    shapes = [frames["group"][0]().order_by(Col("p")), frames["scan"][0]().order_by(Col("product")),
              frames["join"][0]().order_by(Col("u.first_name")), join_group.order_by(Col("n").desc()).limit(2),
              frames["scan"][0]().limit(1)]
    for lower in lowerings:
        for frame in shapes:
            with pytest.raises(st.StageUnsupported):
                lower(frame.task)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu():
    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    key = (hs.hs_col * 1)()
    key[0].kind, key[0].fixed_len, key[0].data = hs.I32, -1, 4096  # never dereferenced by the checks
    desc = (C.c_int32 * 1)(0)
    perm = (C.c_int64 * 4)()
    count = C.c_int64(-7)
    ws = (C.c_uint8 * 64)()
    flags = (C.c_uint32 * 1)()

    def call(keys=key, descending=desc, n_keys=1, nrows=4, limit=-1, out_perm=perm, out_count=C.byref(count), work=ws):
        return lib.hs_order_by(None, keys, descending, n_keys, nrows, None, limit, out_perm, out_count, work, flags)

    assert call(keys=None) == 1
    assert call(descending=None) == 1
    assert call(out_perm=None) == 1
    assert call(out_count=None) == 1
    assert call(work=None) == 1
    assert call(nrows=-1) == 1
    assert call(keys=None, descending=None, n_keys=0, limit=-1) == 1  # nothing to do is not a request
    assert call(n_keys=-1) == 1
    assert b"hs_order_by" in lib.hs_last_error()
    assert call(nrows=0) == 0 and count.value == 0
    count.value = -7
    assert call(nrows=0, limit=3) == 0 and count.value == 0
    assert lib.hs_order_by_ws_bytes(0, 1, 1) > 0
    assert lib.hs_order_by_ws_bytes(1 << 20, 2, 3) >= 4 * 8 * (1 << 20)
