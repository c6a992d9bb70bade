"""Window aggregates without a GPU: the model against a brute force straight from the definition, the
grammar against the API, schema types and names, the refusals of the API, the parser, the planner and the stage lowerings,
and the argument checks of hs_window_agg, which are answered before anything is launched."""

from __future__ import annotations

import ctypes as C
import math

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
from tests.window_agg_model import FRAMES, brute_force, same, window_agg_model


def T(name="t"):
    return DataFrame(object()).table(name)


ORDERS = lambda: load_golden("e2e_join_select")["paths"]["orders"]  # noqa: E731 - user_id, product, quantity, price ...


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_the_model_on_a_hand_written_case():
    part = ["a", "b", "a", "a", "b", "a"]
    key = [5, 1, 5, 3, 1, 9]
    v = [10, 20, 30, 40, 50, 60]
    # 'a' in order: row 3 (3), rows 0 and 2 (5, 5: peers, input order), row 5 (9); 'b': rows 1 and 4 (peers)
    assert window_agg_model(6, [part], [(key, True)], v, "rows")["sum"] == [50, 20, 80, 40, 70, 140]
    assert window_agg_model(6, [part], [(key, True)], v, "range")["sum"] == [80, 70, 80, 40, 70, 140]
    assert window_agg_model(6, [part], [(key, True)], v, "partition")["sum"] == [140, 70, 140, 140, 70, 140]
    assert window_agg_model(6, [part], [(key, True)], v, "range")["count"] == [3, 2, 3, 1, 2, 4]
    assert window_agg_model(6, [part], [(key, False)], v, "rows")["max"] == [60, 20, 60, 60, 50, 60]
    assert window_agg_model(6, [part], [], v, "rows")["min"] == [10, 20, 10, 10, 20, 10]       # no ORDER BY: input order
    assert window_agg_model(6, [], [], v, "rows")["sum"] == [10, 30, 60, 100, 150, 210]
    assert window_agg_model(0, [[]], [([], True)], [], "range")["sum"] == []


def test_the_model_orders_nan_last_and_adds_as_ieee_does():
    nan, inf = math.nan, math.inf
    v = [1.5, nan, -0.0, inf, 0.0, -inf]
    got = window_agg_model(6, [], [], v, "rows")
    assert [same(a, b) for a, b in zip(got["sum"], [1.5, nan, nan, nan, nan, nan])] == [True] * 6
    assert [same(a, b) for a, b in zip(got["max"], [1.5, nan, nan, nan, nan, nan])] == [True] * 6
    assert got["min"][:5] == [1.5, 1.5, -0.0, -0.0, -0.0] and got["min"][5] == -inf
    only = window_agg_model(3, [], [], [inf, 2.0, -inf], "rows")["sum"]
    assert only[:2] == [inf, inf] and math.isnan(only[2])
    assert math.isnan(window_agg_model(2, [], [], [nan, nan], "partition")["min"][0])


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_the_brute_force(seed, frame):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41))
    part = [rng.integers(0, 4, n).tolist()] if seed % 3 else []
    order = [] if seed == 4 else [(rng.integers(0, 5, n).tolist(), bool(seed % 2))]
    if seed == 5:
        order.append((rng.choice([0.0, -0.0, 1.5, math.nan], n).tolist(), True))
    ints = [int(x) for x in rng.integers(-(1 << 31), 1 << 31, n)]
    floats = [float(np.float32(x)) for x in rng.normal(0, 1e6, n) * rng.choice([1e-30, 1.0, 1e30], n)]
    special = [float(x) for x in rng.choice([math.nan, math.inf, -math.inf, -0.0, 0.0, 2.5, -7.0], n)]
    for values in (ints, floats, special):
        got, want = window_agg_model(n, part, order, values, frame), brute_force(n, part, order, values, frame)
        for k in want:
            assert all(same(a, b) for a, b in zip(got[k], want[k])), (k, got[k], want[k])


# ---- grammar and API ---------------------------------------------------------------------------------------------------
OVER = dict(partition_by=[Col("k")], order_by=[Col("o").desc()])
CASES = [
    ("SELECT k, v, SUM(v) OVER (PARTITION BY k) AS t FROM 't';",
     lambda: T().select(Col("k"), Col("v")).window(F.sum(Col("v")).over(partition_by=[Col("k")]).alias("t"))),
    ("SELECT k, o, v, SUM(v) OVER (PARTITION BY k ORDER BY o DESC) FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.sum(Col("v")).over(**OVER))),
    ("SELECT k, o, v, AVG(v)  OVER( PARTITION BY k  ORDER BY o DESC  ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW ) AS a FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.avg(Col("v")).over(**OVER, rows=True).alias("a"))),
    ("SELECT k, o, MIN(o) OVER (ORDER BY o ROWS UNBOUNDED PRECEDING), MAX(o) OVER (ORDER BY o RANGE UNBOUNDED PRECEDING) FROM 't';",
     lambda: T().select(Col("k"), Col("o")).window(F.min(Col("o")).over(order_by=[Col("o")], rows=True),
                                                   F.max(Col("o")).over(order_by=[Col("o")]))),
    ("SELECT k, COUNT() OVER (ROWS UNBOUNDED PRECEDING) AS n, COUNT() OVER (RANGE BETWEEN UNBOUNDED PRECEDING) AS m FROM 't';",
     lambda: T().select(Col("k")).window(F.count().over(rows=True).alias("n"), F.count().over().alias("m"))),
    ("SELECT DISTINCT k, v, AVG(v) OVER (PARTITION BY k) FROM 't' QUALIFY v > avg_v ORDER BY k LIMIT 5;",
     lambda: T().select(Col("k"), Col("v")).window(F.avg(Col("v")).over(partition_by=[Col("k")]))
     .qualify(Col("v") > Col("avg_v")).distinct().order_by(Col("k")).limit(5)),
    ("SELECT k, SUM(v) AS s, SUM(s) OVER (ORDER BY k) AS running FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.sum(Col("v")).alias("s")).select(Col("k"), Col("s"))
     .window(F.sum(Col("s")).over(order_by=[Col("k")]).alias("running"))),
    ("SELECT k, ROW_NUMBER() OVER (ORDER BY k) AS rn, COUNT() OVER (ORDER BY k) FROM 't';",
     lambda: T().select(Col("k")).window(F.row_number().over(order_by=[Col("k")]).alias("rn"), F.count().over(order_by=[Col("k")]))),
]


@pytest.mark.parametrize("sql,build", CASES, ids=[f"{i}" for i in range(len(CASES))])
def test_text_builds_the_same_tree_as_the_api(sql, build):
    got, want = parse_sql(sql, object()).task, build().task
    assert type(got) is t.SortTask and got.windows and type(got.parent_task) is not t.SortTask  # ONE task carries all
    assert render(got) == render(want) and repr(got) == repr(want)
    assert [(w.kind, str(w.arg), w.frame, w.name) for w in got.windows] == [(w.kind, str(w.arg), w.frame, w.name) for w in want.windows]


def test_every_spelling_of_the_frame_clause():
    frames = {"": "range", " ROWS UNBOUNDED PRECEDING": "rows", " ROWS BETWEEN UNBOUNDED PRECEDING": "rows",
              " ROWS UNBOUNDED PRECEDING AND CURRENT ROW": "rows", " ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": "rows",
              " RANGE UNBOUNDED PRECEDING": "range", " RANGE BETWEEN UNBOUNDED PRECEDING": "range",
              " RANGE UNBOUNDED PRECEDING AND CURRENT ROW": "range", " RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": "range"}
    for clause, frame in frames.items():
        item = parse_sql(f"SELECT v, SUM(v) OVER (ORDER BY v{clause}) FROM 't';", object()).task.windows[0]
        assert (item.kind, item.frame, item.name) == ("sum", frame, "sum_v")
        bare = parse_sql(f"SELECT v, SUM(v) OVER ({clause.strip()}) FROM 't';", object()).task.windows[0]
        # without ORDER BY every row is a peer: RANGE is the whole partition
        assert bare.frame == ("rows" if frame == "rows" else "partition") and bare.order_by == []
    for other in ("ROWS 3 PRECEDING", "ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING", "ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
                  "GROUPS UNBOUNDED PRECEDING", "RANGE UNBOUNDED FOLLOWING"):
        with pytest.raises(SqlSyntaxError):
            parse_sql(f"SELECT v, SUM(v) OVER (ORDER BY v {other}) FROM 't';", object())


def test_a_frame_on_a_ranking_function_is_refused():
    for text in ("SELECT a, RANK() OVER (ORDER BY a ROWS UNBOUNDED PRECEDING) FROM 't';",
                 "SELECT a, ROW_NUMBER() OVER (RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW) FROM 't';"):
        with pytest.raises(ValueError, match="takes no frame clause"):
            parse_sql(text, object())
    with pytest.raises(ValueError, match="takes no frame clause"):
        F.dense_rank().over(order_by=[Col("a")], rows=True)


def test_a_window_only_select_list_is_no_global_aggregate_and_group_by_runs_below_the_window():
    task = parse_sql(f"SELECT product, quantity, SUM(quantity) OVER (PARTITION BY product) AS t FROM '{ORDERS()}';", object()).task
    assert type(task.parent_task) is t.ProjectTask and [c.name for c in task.parent_task.columns] == ["product", "quantity"]
    assert [name for name, _ in task.validate_schema()] == ["product", "quantity", "t"]
    text = f"SELECT product, SUM(quantity) AS s, SUM(s) OVER (ORDER BY product) AS running FROM '{ORDERS()}' GROUP BY product;"
    task = parse_sql(text, object()).task
    assert render(task)[1:] == render(parse_sql(f"SELECT product, SUM(quantity) AS s FROM '{ORDERS()}' GROUP BY product;", object()).task)
    assert [(n, str(ty)) for n, ty in task.validate_schema()] == [("product", "STRING"), ("s", "INTEGER"), ("running", "INTEGER")]
    with pytest.raises(SemanticError, match="at least one column"):
        parse_sql("SELECT SUM(v) OVER () FROM 't';", object())
    # an aggregate WITHOUT OVER next to a plain column is what it was
    with pytest.raises(Exception, match="Without GROUP BY"):
        parse_sql("SELECT k, SUM(v), SUM(v) OVER () AS w FROM 't';", object())


def test_schema_types_and_default_names_per_function():
    base = lambda: T(ORDERS()).select(Col("product"), Col("quantity"), Col("price"))  # noqa: E731 - STRING, INTEGER, FLOAT
    items = [F.count().over(), F.sum(Col("quantity")).over(), F.sum(Col("price")).over(), F.avg(Col("quantity")).over(),
             F.avg(Col("price")).over(), F.min(Col("quantity")).over(), F.max(Col("price")).over(), F.row_number().over()]
    schema = base().window(*items).task.validate_schema()
    assert [(n, str(ty)) for n, ty in schema[3:]] == [
        ("count", "INTEGER"), ("sum_quantity", "INTEGER"), ("sum_price", "FLOAT"), ("avg_quantity", "FLOAT"), ("avg_price", "FLOAT"),
        ("min_quantity", "INTEGER"), ("max_price", "FLOAT"), ("row_number", "INTEGER")]
    twice = base().window(F.sum(Col("price")).over(), F.sum(Col("price")).over(order_by=[Col("price")]))
    with pytest.raises(ValueError, match="Duplicate.*sum_price"):
        twice.task.validate_schema()
    with pytest.raises(ValueError, match="Duplicate.*quantity"):
        base().window(F.count().over().alias("quantity")).task.validate_schema()
    assert str(F.sum(Col("v")).over(partition_by=[Col("k")], order_by=[Col("o").desc()], rows=True).alias("s")) == \
        "SUM(v) OVER (PARTITION BY k ORDER BY o DESC ROWS UNBOUNDED PRECEDING) AS s"
    assert str(F.count().over(order_by=[Col("o")])) == "COUNT() OVER (ORDER BY o ASC RANGE UNBOUNDED PRECEDING) AS count"
    assert str(F.max(Col("v")).over()) == "MAX(v) OVER () AS max_v"


def test_two_items_of_one_spec_share_a_sort():
    a = F.sum(Col("v")).over(**OVER, rows=True)
    b = F.rank().over(**OVER)
    c = F.count().over(partition_by=[Col("k")])
    assert a.spec() == b.spec() != c.spec() and len({i.spec() for i in (a, b, c)}) == 2


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_the_argument_is_a_plain_numeric_column_of_the_result():
    base = lambda: T(ORDERS()).select(Col("product"), Col("quantity"))  # noqa: E731
    with pytest.raises(TypeError, match='"product" is STRING'):
        base().window(F.max(Col("product")).over()).task.validate_schema()
    stamps = load_golden("q1_multiblock")["paths"]["lineitem"]
    with pytest.raises(TypeError, match='"l_shipdate"'):
        T(stamps).select(Col("l_shipdate")).window(F.min(Col("l_shipdate")).over()).task.validate_schema()
    with pytest.raises(ValueError, match='"price" not found'):  # not selected: the error a key raises
        base().window(F.sum(Col("price")).over()).task.validate_schema()
    with pytest.raises(ValueError, match='"n" not found'):     # another window item is no argument
        base().window(F.count().over().alias("n"), F.sum(Col("n")).over().alias("m")).task.validate_schema()
    with pytest.raises(ValueError, match="plain columns.*alias"):
        F.sum(Col("a") + 1).over()
    with pytest.raises(ValueError, match="plain columns.*alias"):
        F.sum(Lit(2)).over()
    with pytest.raises(ValueError, match="plain columns"):
        F.sum(Col("a")).over(order_by=[Col("a") * 2])
    with pytest.raises(ValueError, match="COUNT\\(DISTINCT\\)"):
        F.count_distinct(Col("a")).over()
    with pytest.raises(SemanticError, match="alias the expression in the select list"):
        parse_sql("SELECT a, SUM(a + 1) OVER (ORDER BY a) FROM 't';", object())
    with pytest.raises(ValueError, match="over"):
        T().select(Col("a")).window(F.sum(Col("a")))  # no .over(...): an AggCol is no window item
    with pytest.raises(ValueError, match="one of"):
        WindowItem("median", Col("a"))


def test_the_limits_of_the_ranking_items_hold():
    items = [F.sum(Col("a")).over(order_by=[Col("a")]).alias(f"w{i}") for i in range(9)]
    with pytest.raises(ValueError, match="at most 8 window items"):
        T().select(Col("a")).window(*items)
    with pytest.raises(ValueError, match="at most 12"):
        T().select(Col("a")).window(F.count().over(partition_by=[Col("a")] * 7, order_by=[Col("a")] * 6))
    with pytest.raises(SemanticError, match="QUALIFY.*no window item"):
        parse_sql("SELECT a, SUM(a) AS s FROM 't' GROUP BY a QUALIFY s > 1;", object())


def test_a_windowed_aggregate_below_another_operation_is_refused_when_planned():
    below = _golden_frames()["scan"]().window(F.sum(Col("quantity")).over(order_by=[Col("product")])).filter(Col("quantity") > 1)
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(below.task)


KEYS = {"scan": "product", "group": "p", "join": "u.first_name", "join_group": "n"}


def test_all_five_stage_lowerings_refuse_a_plan_with_a_window_aggregate():
    from minispark_amd import stage as st

    lowerings = [st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                 st.lower_join_group_stage_plan]
    for lower in lowerings:
        for shape, key in KEYS.items():
            frame = _golden_frames()[shape]().window(F.count().over(order_by=[Col(key)], rows=True).alias("c"))
            with pytest.raises(st.StageUnsupported):
                lower(frame.task)


def test_the_windowed_task_adds_a_float_column_in_the_result_stage():
    frame = _golden_frames()["group"]().window(F.avg(Col("p")).over().alias("mean")).qualify(Col("p") > Col("mean"))
    last = PhysicalPlan.generate_physical_plan(frame.task).stages[-1]
    sort = next(x for x in last.consumers if type(x).__name__ == "SortTask")
    assert [str(ty) for _, ty in sort.inferred_schema][-1] == "FLOAT" and last.writer.inferred_schema[-1][0] == "mean"


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

    def call(n_part=1, n_keys=2, nrows=4, funcs=(hs.WIN_SUM,), frames=(hs.WIN_FRAME_RANGE,), kinds=(hs.I32,), outs=out, work=ws,
             keys=key, no_values=False, no_frames=False):
        n = len(funcs)
        fs = (C.c_int32 * max(n, 1))(*funcs)
        fr = (C.c_int32 * max(n, 1))(*(list(frames) * n)[:n])
        vals = (hs.hs_col * max(n, 1))()
        for i in range(n):
            vals[i].kind, vals[i].fixed_len, vals[i].data = (list(kinds) * n)[i], -1, 4096
        return lib.hs_window_agg(None, keys, desc, n_part, n_keys, nrows, fs, None if no_frames else fr,
                                 None if no_values else vals, n, outs, work, None)

    assert call(n_keys=13) == 2 and b"12" in lib.hs_last_error()
    assert call(nrows=1 << 31) == 2 and b"2^31" in lib.hs_last_error()
    assert call(funcs=[hs.WIN_SUM] * 9) == 2 and b"8" in lib.hs_last_error()
    assert call(funcs=(8,)) == 1 and b"function 8" in lib.hs_last_error()
    assert call(funcs=(-1,)) == 1
    assert call(funcs=(hs.WIN_COUNT, hs.WIN_MIN), frames=(0, 3)) == 1 and b"item 1: frame 3" in lib.hs_last_error()
    assert call(funcs=(hs.WIN_COUNT,), no_frames=True) == 1 and b"item 0" in lib.hs_last_error()
    for kind in (hs.I64, hs.F64, hs.STR, hs.U8, 6, 7, 16, 17, 0x100 | hs.I32):  # other types, narrow, virtual, pair-indexed
        assert call(funcs=(hs.WIN_ROW_NUMBER, hs.WIN_AVG), kinds=(hs.I32, kind)) == 1
        assert b"item 1" in lib.hs_last_error() and str(kind).encode() in lib.hs_last_error()
    assert call(no_values=True) == 1 and b"item 0" in lib.hs_last_error()
    assert call(n_part=2, funcs=(hs.WIN_SUM, hs.WIN_RANK)) == 1 and b"order key" in lib.hs_last_error()
    assert call(n_part=3) == 1 and call(n_part=-1) == 1 and call(nrows=-1) == 1 and call(funcs=()) == 1 and call(outs=None) == 1
    assert call(work=None) == 1 and call(keys=None) == 1
    # ranking items read neither a frame nor an argument; COUNT no argument; without rows nothing is launched
    assert call(nrows=0, funcs=(hs.WIN_ROW_NUMBER, hs.WIN_COUNT), kinds=(hs.STR,)) == 0
    assert call(nrows=0, funcs=(hs.WIN_RANK,), frames=(9,), no_values=True) == 0 and call(nrows=0, n_part=2) == 0
    assert (lib.hs_window_agg_ws_bytes(1 << 20, 2, 3, 1) >= lib.hs_window_ws_bytes(1 << 20, 2, 3) + (16 << 20)
            and lib.hs_window_agg_ws_bytes(1 << 20, 2, 3, 8) == lib.hs_window_agg_ws_bytes(1 << 20, 2, 3, 1))
    assert (hs.WIN_COUNT, hs.WIN_SUM, hs.WIN_AVG, hs.WIN_MIN, hs.WIN_MAX) == (3, 4, 5, 6, 7)
    assert (hs.WIN_FRAME_PARTITION, hs.WIN_FRAME_RANGE, hs.WIN_FRAME_ROWS) == (0, 1, 2)
