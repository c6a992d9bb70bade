"""Sliding window frames without a GPU: ROWS BETWEEN n PRECEDING AND m FOLLOWING in the grammar and the
API, the texts that must keep failing, schema types, the refusals, the model (tests/window_frame_model.py) against a second
brute force, and the argument checks of hs_window_frames, which are answered before anything is launched."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from minispark_amd import tasks as t
from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SemanticError, SqlSyntaxError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col
from minispark_amd.sql import Functions as F
from tests.conftest import load_golden
from tests.test_distinct_cpu import _golden_frames
from tests.test_parser import render
from tests.window_agg_model import _order_key, same
from tests.window_frame_model import COLUMNS, window_frame_exact, window_frame_model
from tests.window_model import codes


def T(name="t"):
    return DataFrame(object()).table(name)


ORDERS = lambda: load_golden("e2e_join_select")["paths"]["orders"]  # noqa: E731 - user_id, product, quantity, price ...
HEADS = ("SUM", "AVG", "MIN", "MAX", "COUNT", "FIRST_VALUE", "LAST_VALUE")


def call_of(head):
    return "COUNT()" if head == "COUNT" else f"{head}(v)"


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_the_model_on_a_hand_written_case():
    part = ["a", "b", "a", "a", "b", "a"]
    key = [5, 1, 5, 3, 1, 9]
    v = [10, 20, 30, 40, 50, 60]
    # 'a' in order: row 3 (3), rows 0 and 2 (5, 5: ties in input order), row 5 (9); 'b': rows 1 and 4
    got = window_frame_model(6, [part], [(key, True)], v, 1, 0)
    assert got["sum"] == [50, 20, 40, 40, 70, 90] and got["count"] == [2, 1, 2, 1, 2, 2]
    assert got["first"] == [3, 1, 0, 3, 1, 2] and got["last"] == [0, 1, 2, 3, 4, 5]
    got = window_frame_model(6, [part], [(key, True)], v, 1, 1)
    assert got["sum"] == [80, 70, 100, 50, 70, 90] and got["max"] == [40, 50, 60, 40, 50, 60] and got["min"] == [10, 20, 10, 10, 20, 30]
    assert got["last"] == [2, 4, 5, 0, 4, 5]
    assert window_frame_model(6, [part], [(key, True)], v, 0, 0)["sum"] == v                      # CURRENT ROW alone
    assert window_frame_model(6, [part], [(key, True)], v, 99, 99)["sum"] == [140, 70, 140, 140, 70, 140]  # the partition
    assert window_frame_model(6, [], [], v, 0, 2)["sum"] == [60, 90, 120, 150, 110, 60]              # no keys: input order
    assert window_frame_model(0, [[]], [([], True)], [], 1, 1)["sum"] == []


def test_a_nan_is_seen_by_exactly_the_rows_whose_frame_holds_it():
    nan, inf = math.nan, math.inf
    got = window_frame_model(7, [], [], [1.0, 2.0, nan, 4.0, inf, -inf, 7.0], 1, 0)
    assert [same(a, b) for a, b in zip(got["sum"], [1.0, 3.0, nan, nan, inf, nan, -inf])] == [True] * 7
    assert [same(a, b) for a, b in zip(got["max"], [1.0, 2.0, nan, nan, inf, inf, 7.0])] == [True] * 7
    assert got["min"][2] == 2.0 and got["min"][5] == -inf
    zeros = window_frame_model(4, [], [], [-0.0, 0.0, -0.0, -0.0], 1, 1)
    assert all(v == 0.0 for k in ("sum", "min", "max") for v in zeros[k])


def second_brute_force(n, partition, order, values, preceding, following):
    """Straight from the definition, written another way: per row, the rows of its partition sorted by (keys, input
    place), the row's place among them, the slice around it."""
    part = [codes(v) for v in partition]
    keys = [codes(v) if ascending else -codes(v) for v, ascending in order]
    is_float = any(isinstance(v, float) for v in values)
    out = {k: [] for k in COLUMNS}
    for i in range(n):
        mates = sorted((r for r in range(n) if all(p[r] == p[i] for p in part)), key=lambda r: (tuple(k[r] for k in keys), r))
        j = mates.index(i)
        rows = mates[max(0, j - preceding):j + following + 1]
        cells = [values[r] for r in rows]
        if not is_float:
            total = sum(cells)
        elif all(math.isfinite(c) for c in cells):
            total = math.fsum(cells)
        elif any(math.isnan(c) for c in cells) or (math.inf in cells and -math.inf in cells):
            total = math.nan
        else:
            total = math.inf if math.inf in cells else -math.inf
        mass = math.fsum(abs(c) for c in cells) if is_float else float(sum(abs(c) for c in cells))
        for k, v in zip(COLUMNS, (total, len(cells), mass, min(cells, key=_order_key), max(cells, key=_order_key), rows[0], rows[-1])):
            out[k].append(v)
    return out


@pytest.mark.parametrize("seed", range(8))
def test_the_model_is_a_second_brute_force_and_the_fast_model_is_the_model(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41))
    part = [rng.integers(0, 4, n).tolist()] if seed % 3 else []
    order = [] if seed == 4 else [(rng.integers(0, 5, n).tolist(), bool(seed % 2))]  # ties; descending for odd seeds
    if seed == 5:
        order.append((rng.choice([0.0, -0.0, 1.5, math.nan], n).tolist(), True))
    ints = [int(x) for x in rng.integers(-(1 << 31), 1 << 31, n)]
    floats = [float(np.float32(x)) for x in rng.normal(0, 1e6, n) * rng.choice([1e-30, 1.0, 1e30], n)]
    special = [float(x) for x in rng.choice([math.nan, math.inf, -math.inf, -0.0, 0.0, 2.5, -7.0], n)]
    for preceding, following in ((0, 0), (1, 0), (0, 1), (3, 2), (n + 5, 0), (0, n + 5), (n + 5, n + 5), (2, 100)):
        for values in (ints, floats, special):
            got = window_frame_model(n, part, order, values, preceding, following)
            want = second_brute_force(n, part, order, values, preceding, following)
            fast = window_frame_exact(n, part, order, values, preceding, following)
            for k in COLUMNS:
                if k == "abs":  # a plain f64 running sum in the model: equal to rounding, and non-finite together
                    close = lambda a, b: a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= 1e-12 * abs(b)) or \
                        not (math.isfinite(a) or math.isfinite(b))  # noqa: E731
                    assert all(close(a, b) and close(c, b) for a, b, c in zip(got[k], want[k], fast[k])), (k, got[k], want[k], fast[k])
                else:
                    assert all(same(a, b) for a, b in zip(got[k], want[k])), (k, preceding, following, got[k], want[k])
                    assert all(same(a, b) for a, b in zip(fast[k], want[k])), (k, preceding, following, fast[k], want[k])
            if preceding == n + 5 == following:  # wider than every partition: the partition frame
                whole = window_frame_model(n, part, order, values, 1 << 30, (1 << 31) - 1)
                assert all(same(a, b) for k in COLUMNS if k != "abs" for a, b in zip(got[k], whole[k]))


# ---- grammar and API ---------------------------------------------------------------------------------------------------
SPELLINGS = {"ROWS BETWEEN 2 PRECEDING AND CURRENT ROW": (2, 0), "ROWS BETWEEN CURRENT ROW AND 3 FOLLOWING": (0, 3),
             "ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING": (1, 1), "ROWS BETWEEN CURRENT ROW AND CURRENT ROW": (0, 0),
             "ROWS BETWEEN 0 PRECEDING AND 0 FOLLOWING": (0, 0), "ROWS  BETWEEN  6 PRECEDING  AND  CURRENT  ROW": (6, 0),
             "ROWS BETWEEN 2147483647 PRECEDING AND 2147483647 FOLLOWING": ((1 << 31) - 1, (1 << 31) - 1)}


@pytest.mark.parametrize("head", HEADS)
def test_every_accepted_spelling_builds_the_item(head):
    for clause, (n, m) in SPELLINGS.items():
        name = "count" if head == "COUNT" else f"{head.lower()}_v"
        for over in (f"ORDER BY v {clause}", f"PARTITION BY k ORDER BY v DESC {clause}", f"PARTITION BY k {clause}", clause):
            item = parse_sql(f"SELECT k, v, {call_of(head)} OVER ({over}) FROM 't';", object()).task.windows[0]
            assert (item.kind, item.frame, item.preceding, item.following, item.name) == (head.lower(), "between", n, m, name)
            assert (item.order_by != []) == ("ORDER BY" in over) and (item.partition_by != []) == ("PARTITION" in over)
    aliased = parse_sql(f"SELECT v, {call_of(head)} OVER (ORDER BY v ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) AS w FROM 't';", object())
    assert aliased.task.windows[0].name == "w"
    # every other frame keeps preceding / following unset
    older = parse_sql(f"SELECT v, {call_of(head)} OVER (ORDER BY v ROWS UNBOUNDED PRECEDING) FROM 't';", object()).task.windows[0]
    assert (older.frame, older.preceding, older.following) == ("rows", None, None)


OVER = dict(partition_by=[Col("k")], order_by=[Col("o").desc()])
CASES = [
    ("SELECT k, o, v, AVG(v) OVER (PARTITION BY k ORDER BY o DESC ROWS BETWEEN 6 PRECEDING AND CURRENT ROW) AS week FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.avg(Col("v")).over(**OVER, rows=(6, 0)).alias("week"))),
    ("SELECT o, v, SUM(v) OVER (ORDER BY o ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING), MIN(v) OVER (ORDER BY o ROWS BETWEEN CURRENT ROW "
     "AND 9 FOLLOWING), COUNT() OVER (ORDER BY o ROWS BETWEEN 2 PRECEDING AND 2 FOLLOWING) FROM 't';",
     lambda: T().select(Col("o"), Col("v")).window(F.sum(Col("v")).over(order_by=[Col("o")], rows=(1, 1)),
                                                   F.min(Col("v")).over(order_by=[Col("o")], rows=(0, 9)),
                                                   F.count().over(order_by=[Col("o")], rows=(2, 2)))),
    ("SELECT k, v, FIRST_VALUE(v) OVER (PARTITION BY k ROWS BETWEEN 3 PRECEDING AND CURRENT ROW) AS f, "
     "LAST_VALUE(v) OVER (PARTITION BY k ROWS BETWEEN CURRENT ROW AND 3 FOLLOWING) AS l FROM 't';",
     lambda: T().select(Col("k"), Col("v")).window(F.first_value(Col("v")).over(partition_by=[Col("k")], rows=(3, 0)).alias("f"),
                                                   F.last_value(Col("v")).over(partition_by=[Col("k")], rows=[0, 3]).alias("l"))),
    ("SELECT DISTINCT k, v, MAX(v) OVER (PARTITION BY k ORDER BY v ROWS BETWEEN 2 PRECEDING AND 2 FOLLOWING) AS top, "
     "ROW_NUMBER() OVER (PARTITION BY k ORDER BY v) AS rn FROM 't' QUALIFY v = top ORDER BY k LIMIT 5;",
     lambda: T().select(Col("k"), Col("v")).window(
         F.max(Col("v")).over(partition_by=[Col("k")], order_by=[Col("v")], rows=(2, 2)).alias("top"),
         F.row_number().over(partition_by=[Col("k")], order_by=[Col("v")]).alias("rn"))
     .qualify(Col("v") == Col("top")).distinct().order_by(Col("k")).limit(5)),
    ("SELECT k, SUM(v) AS s, SUM(s) OVER (ORDER BY k ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) AS pair FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.sum(Col("v")).alias("s")).select(Col("k"), Col("s"))
     .window(F.sum(Col("s")).over(order_by=[Col("k")], rows=(1, 0)).alias("pair"))),
]


@pytest.mark.parametrize("sql,build", CASES, ids=[f"{i}" for i in range(len(CASES))])
def test_text_builds_the_same_tree_as_the_api_and_prints_the_same(sql, build):
    got, want = parse_sql(sql, object()).task, build().task
    assert type(got) is t.SortTask and got.windows and type(got.parent_task) is not t.SortTask  # ONE task carries all
    assert render(got) == render(want) and repr(got) == repr(want) and got.describe() == want.describe()
    seen = lambda w: (w.kind, str(w.arg), w.frame, w.preceding, w.following, w.name, str(w))  # noqa: E731
    assert [seen(w) for w in got.windows] == [seen(w) for w in want.windows]


def test_how_a_sliding_item_prints():
    item = F.sum(Col("v")).over(partition_by=[Col("k")], order_by=[Col("o").desc()], rows=(2, 0)).alias("s")
    assert str(item) == repr(item) == "SUM(v) OVER (PARTITION BY k ORDER BY o DESC ROWS BETWEEN 2 PRECEDING AND CURRENT ROW) AS s"
    assert str(F.count().over(rows=(0, 4))) == "COUNT() OVER (ROWS BETWEEN CURRENT ROW AND 4 FOLLOWING) AS count"
    assert str(F.last_value(Col("v")).over(order_by=[Col("v")], rows=(1, 1))) == \
        "LAST_VALUE(v) OVER (ORDER BY v ASC ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING) AS last_value_v"
    assert str(F.min(Col("v")).over(rows=(0, 0))) == "MIN(v) OVER (ROWS BETWEEN CURRENT ROW AND CURRENT ROW) AS min_v"
    frame = T().select(Col("k"), Col("v")).window(item)
    assert "ROWS BETWEEN 2 PRECEDING AND CURRENT ROW" in frame.task.describe()
    text = f"SELECT k, o, v, {str(item)} FROM 't';"  # what an item prints parses back to the item
    assert str(parse_sql(text, object()).task.windows[0]) == str(item)
    again = F.sum(Col("v")).over(rows=(2, 3)).over(order_by=[Col("v")])  # a second over() replaces the first
    assert (again.frame, again.preceding, again.following) == ("range", None, None)


def test_items_of_one_spec_share_a_sort_whatever_their_frames():
    a = F.sum(Col("v")).over(**OVER, rows=(3, 3))
    b = F.sum(Col("v")).over(**OVER, rows=True).alias("b")
    c = F.rank().over(**OVER)
    d = F.avg(Col("v")).over(**OVER, rows=(0, 1))
    assert a.spec() == b.spec() == c.spec() == d.spec() and a.name == "sum_v" and d.name == "avg_v"


# ---- what stays refused ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_the_pinned_texts_keep_failing(head):
    """BETWEEN is mandatory, both ends are finite, GROUPS and a RANGE of values do not exist."""
    short = SemanticError if head.endswith("_VALUE") else SqlSyntaxError  # what each head raised before this frame existed
    for clause, error in (("ROWS 3 PRECEDING", short), ("ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING", None),
                          ("ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING", None), ("GROUPS UNBOUNDED PRECEDING", None),
                          ("RANGE UNBOUNDED FOLLOWING", None), ("RANGE BETWEEN 3 PRECEDING AND CURRENT ROW", None),
                          ("ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING", None), ("ROWS BETWEEN 2 PRECEDING AND 1 PRECEDING", None),
                          ("ROWS BETWEEN -1 PRECEDING AND CURRENT ROW", None), ("ROWS BETWEEN 1.5 PRECEDING AND CURRENT ROW", None),
                          ("ROWS BETWEEN 2 PRECEDING", None), ("ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING", None),
                          ("GROUPS BETWEEN 1 PRECEDING AND 1 FOLLOWING", None)):
        with pytest.raises((SqlSyntaxError, SemanticError) if error is None else error):
            parse_sql(f"SELECT v, {call_of(head)} OVER (ORDER BY v {clause}) FROM 't';", object())


def test_the_rejections_the_older_tests_pin_raise_what_they_raised():
    for other in ("ROWS 3 PRECEDING", "ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING", "ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
                  "GROUPS UNBOUNDED PRECEDING", "RANGE UNBOUNDED FOLLOWING"):
        with pytest.raises(SqlSyntaxError):
            parse_sql(f"SELECT v, SUM(v) OVER (ORDER BY v {other}) FROM 't';", object())
    for head in ("FIRST_VALUE", "LAST_VALUE"):
        with pytest.raises(SemanticError, match=f"^Unsupported function: {head}$"):
            parse_sql(f"SELECT v, {head}(v) OVER (ORDER BY v ROWS 3 PRECEDING) FROM 't';", object())
    with pytest.raises(Exception, match="GROUP BY"):  # the unparenthesised GROUP BY takes one column, as ever
        parse_sql("SELECT a, b, SUM(v) AS s FROM 't' GROUP BY a, b;", object())


def test_functions_that_take_no_frame_refuse_the_sliding_one_too():
    clause = "ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING"
    for call in ("ROW_NUMBER()", "RANK()", "DENSE_RANK()", "LAG(v, 1, 0)", "LEAD(v, 1, 0)", "NTILE(4)"):
        with pytest.raises(ValueError, match="takes no frame clause"):
            parse_sql(f"SELECT v, {call} OVER (ORDER BY v {clause}) FROM 't';", object())
    for item in (F.row_number(), F.rank(), F.dense_rank(), F.lag(Col("v"), 1, 0), F.lead(Col("v"), 1, 0), F.ntile(4)):
        with pytest.raises(ValueError, match="takes no frame clause"):
            item.over(order_by=[Col("v")], rows=(1, 1))
        with pytest.raises(ValueError, match="takes no frame clause"):
            item.over(order_by=[Col("v")], rows=(0, 0))


def test_bad_pairs_are_value_errors():
    for bad in ((True, 1), (1, False), (-1, 0), (0, -1), (1 << 31, 0), (0, 1 << 31), (1,), (1, 2, 3), (1.0, 2), ("1", 2), 3, None,
                "rows", (None, 1)):
        for build in (lambda: F.sum(Col("v")), F.count, lambda: F.first_value(Col("v")), F.row_number):
            with pytest.raises(ValueError, match="rows=|takes no frame clause"):
                build().over(order_by=[Col("v")], rows=bad)
    with pytest.raises(ValueError, match="rows="):
        parse_sql("SELECT v, SUM(v) OVER (ORDER BY v ROWS BETWEEN 2147483648 PRECEDING AND CURRENT ROW) FROM 't';", object())
    ok = F.sum(Col("v")).over(rows=((1 << 31) - 1, (1 << 31) - 1))
    assert (ok.preceding, ok.following) == ((1 << 31) - 1,) * 2


def test_schema_types_names_and_argument_errors():
    base = lambda: T(ORDERS()).select(Col("product"), Col("quantity"), Col("price"))  # noqa: E731 - STRING, INTEGER, FLOAT
    items = [F.count().over(rows=(1, 1)), F.sum(Col("quantity")).over(rows=(1, 1)), F.sum(Col("price")).over(rows=(1, 1)),
             F.avg(Col("quantity")).over(rows=(1, 1)), F.min(Col("quantity")).over(rows=(0, 2)), F.max(Col("price")).over(rows=(2, 0)),
             F.first_value(Col("price")).over(rows=(2, 0)), F.last_value(Col("quantity")).over(rows=(0, 2))]
    schema = base().window(*items).task.validate_schema()
    assert [(n, str(ty)) for n, ty in schema[3:]] == [
        ("count", "INTEGER"), ("sum_quantity", "INTEGER"), ("sum_price", "FLOAT"), ("avg_quantity", "FLOAT"), ("min_quantity", "INTEGER"),
        ("max_price", "FLOAT"), ("first_value_price", "FLOAT"), ("last_value_quantity", "INTEGER")]
    stamps = load_golden("q1_multiblock")["paths"]["lineitem"]
    shipped = T(stamps).select(Col("l_shipdate")).window(F.first_value(Col("l_shipdate")).over(rows=(1, 0)))
    assert str(shipped.task.validate_schema()[-1][1]) == "TIMESTAMP"
    with pytest.raises(TypeError, match='"product" is STRING'):
        base().window(F.max(Col("product")).over(rows=(1, 1))).task.validate_schema()
    with pytest.raises(TypeError, match='"product" is STRING'):
        base().window(F.last_value(Col("product")).over(rows=(1, 1))).task.validate_schema()
    with pytest.raises(TypeError, match='"l_shipdate"'):
        T(stamps).select(Col("l_shipdate")).window(F.sum(Col("l_shipdate")).over(rows=(1, 1))).task.validate_schema()
    with pytest.raises(ValueError, match="Duplicate.*sum_price"):
        base().window(F.sum(Col("price")).over(rows=(1, 1)), F.sum(Col("price")).over(rows=True)).task.validate_schema()


def test_the_guards_of_the_windowed_task_are_inherited():
    from minispark_amd import stage as st

    item = lambda i=0: F.sum(Col("quantity")).over(order_by=[Col("product")], rows=(1, 1)).alias(f"w{i}")  # noqa: E731
    below = _golden_frames()["scan"]().window(item()).filter(Col("quantity") > 1)
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(below.task)
    with pytest.raises(ValueError, match="at most 8 window items"):
        T().select(Col("product"), Col("quantity")).window(*[item(i) for i in range(9)])
    with pytest.raises(ValueError, match="at most 12"):
        T().select(Col("a")).window(F.count().over(partition_by=[Col("a")] * 7, order_by=[Col("a")] * 6, rows=(1, 1)))
    keys = {"scan": "product", "group": "p", "join": "u.first_name", "join_group": "n"}
    for lower in (st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                  st.lower_join_group_stage_plan):
        for shape, key in keys.items():
            frame = _golden_frames()[shape]().window(F.count().over(order_by=[Col(key)], rows=(2, 2)).alias("c"))
            with pytest.raises(st.StageUnsupported):
                lower(frame.task)


# ---- the engine's call ---------------------------------------------------------------------------------------------------
def test_window_rows_hands_the_offsets_over_and_older_queries_make_the_call_they_made():
    from minispark_amd.constants import ColumnType
    from minispark_amd.execution import HipExecutionEngine

    class Dev:
        def __init__(self):
            self.calls = []

        def resolve(self, batch):
            return batch

        def window(self, batch, part, order, items):
            self.calls.append((part, order, [i.func for i in items], [i.frame for i in items], [i.value for i in items],
                               [i.param for i in items], [i.offsets for i in items]))
            return [f"col{i}" for i in range(len(items))]

    class Batch:
        nrows, cols = 5, ["k", "v"]

    engine = HipExecutionEngine.__new__(HipExecutionEngine)
    engine.dev = Dev()
    engine._quantise_batch = lambda batch, schema: batch
    schema = [("k", ColumnType.INTEGER), ("v", ColumnType.INTEGER)]
    keys = dict(partition_by=[Col("k")], order_by=[Col("v")])

    def run(*items):
        engine.dev.calls.clear()
        task = T().select(Col("k"), Col("v")).window(*items).task
        task.input_schema, task.inferred_schema = schema, [*schema, *[(i.name, ColumnType.INTEGER) for i in items]]
        engine._window_rows(Batch(), task)
        return list(engine.dev.calls)

    calls = run(F.row_number().over(**keys), F.sum(Col("v")).over(**keys, rows=(2, 1)), F.lag(Col("v"), 1, 0).over(**keys),
                F.last_value(Col("v")).over(**keys, rows=(0, 3)).alias("l"))
    assert calls == [([0], [(1, True)], ["row_number", "sum", "lag", "last_value"], [None, "between", None, "between"],
                      [None, 1, 1, 1], [None, None, (1, 0), None], [None, (2, 1), None, (0, 3)])]
    calls = run(F.count().over(**keys, rows=(1, 1)))
    assert calls == [([0], [(1, True)], ["count"], ["between"], [None], [None], [(1, 1)])]
    # without a sliding item: the fields of before, no offsets
    assert run(F.row_number().over(**keys)) == [([0], [(1, True)], ["row_number"], [None], [None], [None], [None])]
    assert run(F.sum(Col("v")).over(**keys, rows=True)) == [([0], [(1, True)], ["sum"], ["rows"], [1], [None], [None])]
    assert run(F.sum(Col("v")).over(**keys), F.lead(Col("v"), 2, 7).over(**keys)) == \
        [([0], [(1, True)], ["sum", "lead"], ["range", None], [1, 1], [None, (2, 7)], [None, None])]


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
    BETWEEN = hs.WIN_FRAME_BETWEEN
    assert BETWEEN == 3

    def call(n_part=1, n_keys=2, nrows=4, funcs=(hs.WIN_SUM,), frames=(BETWEEN,), kinds=(hs.I32,), pre=(1,), fol=(1,), no_pre=False,
             no_fol=False, no_params=True, no_values=False, no_frames=False, entry="hs_window_frames"):
        n = len(funcs)
        fs = (C.c_int32 * max(n, 1))(*funcs)
        fr = (C.c_int32 * max(n, 1))(*(list(frames) * n)[:n])
        vals = (hs.hs_col * max(n, 1))()
        for i in range(n):
            vals[i].kind, vals[i].fixed_len, vals[i].data = (list(kinds) * n)[i], -1, 4096
        params, cells = (C.c_int64 * max(n, 1))(*[1] * n), (C.c_uint64 * max(n, 1))()
        before, after = (C.c_int64 * max(n, 1))(*(list(pre) * n)[:n]), (C.c_int64 * max(n, 1))(*(list(fol) * n)[:n])
        head = (None, key, desc, n_part, n_keys, nrows, fs, None if no_frames else fr, None if no_values else vals)
        if entry == "hs_window_agg":
            return lib.hs_window_agg(*head, n, out, ws, None)
        nav = (None if no_params else params, None if no_params else cells)
        if entry == "hs_window_nav":
            return lib.hs_window_nav(*head, *nav, n, out, ws, None)
        return lib.hs_window_frames(*head, *nav, None if no_pre else before, None if no_fol else after, n, out, ws, None)

    said = lib.hs_last_error
    # what hs_window_nav refuses
    assert call(n_keys=13) == 2 and b"12" in said()
    assert call(nrows=1 << 31) == 2 and b"2^31" in said()
    assert call(funcs=[hs.WIN_SUM] * 9) == 2 and b"8" in said()
    assert call(funcs=(13,)) == 1 and b"function 13" in said() and call(funcs=(-1,)) == 1
    assert call(funcs=(hs.WIN_COUNT, hs.WIN_MIN), frames=(0, 4)) == 1 and b"item 1: frame 4" in said()
    assert call(funcs=(hs.WIN_COUNT,), no_frames=True) == 1 and b"item 0" in said()
    assert call(funcs=(hs.WIN_ROW_NUMBER, hs.WIN_AVG), frames=(0, 3), kinds=(hs.I32, hs.I64)) == 1 and b"item 1" in said()
    assert call(funcs=(hs.WIN_LAG,), frames=(0,)) == 1 and b"params is null" in said()
    assert call(no_values=True) == 1 and b"item 0" in said()
    assert call(n_part=2, funcs=(hs.WIN_SUM, hs.WIN_RANK), frames=(3, 0)) == 1 and b"order key" in said()
    # the offsets
    for bad in (-1, 1 << 31, -(1 << 40), 1 << 62):
        assert call(funcs=(hs.WIN_COUNT, hs.WIN_SUM), pre=(0, bad)) == 1 and b"item 1: preceding" in said() and b"2^31" in said()
        assert call(funcs=(hs.WIN_COUNT, hs.WIN_MAX), fol=(0, bad)) == 1 and b"item 1: following" in said() and b"2^31" in said()
    assert call(funcs=(hs.WIN_ROW_NUMBER, hs.WIN_SUM), frames=(0, 3), no_pre=True) == 1 and b"item 1" in said() and b"preceding is null" in said()
    assert call(funcs=(hs.WIN_ROW_NUMBER, hs.WIN_AVG), frames=(0, 3), no_fol=True) == 1 and b"item 1" in said() and b"following is null" in said()
    assert call(funcs=(hs.WIN_COUNT,), no_fol=True) == 1 and b"item 0" in said()
    # the frame on a function that takes none
    for func in (hs.WIN_ROW_NUMBER, hs.WIN_RANK, hs.WIN_DENSE_RANK, hs.WIN_LAG, hs.WIN_LEAD, hs.WIN_NTILE):
        assert call(funcs=(hs.WIN_COUNT, func), no_params=False) == 1
        assert b"item 1: frame 3" in said() and b"takes no frame" in said()
    # the older entries go on refusing the frame
    assert call(funcs=(hs.WIN_COUNT, hs.WIN_MIN), frames=(0, 3), entry="hs_window_agg") == 1 and b"hs_window_agg: item 1: frame 3" in said()
    assert call(funcs=(hs.WIN_COUNT, hs.WIN_LAST_VALUE), frames=(0, 3), entry="hs_window_nav") == 1
    assert b"hs_window_nav: item 1: frame 3" in said()
    # accepted: without rows nothing is launched, and only the offsets an item reads are looked at
    assert call(nrows=0) == 0 and call(nrows=0, pre=((1 << 31) - 1,), fol=((1 << 31) - 1,)) == 0 and call(nrows=0, pre=(0,), fol=(0,)) == 0
    assert call(nrows=0, funcs=(hs.WIN_FIRST_VALUE,), no_fol=True) == 0 and call(nrows=0, funcs=(hs.WIN_LAST_VALUE,), no_pre=True) == 0
    assert call(nrows=0, funcs=(hs.WIN_FIRST_VALUE,), fol=(-5,), kinds=(hs.I64,)) == 0
    assert call(nrows=0, funcs=(hs.WIN_SUM, hs.WIN_ROW_NUMBER), frames=(2, 0), no_pre=True, no_fol=True) == 0  # no sliding item
    assert call(nrows=0, funcs=(hs.WIN_SUM,), frames=(1,), pre=(-1,), fol=(-1,)) == 0                           # not read
    nav, frames = lib.hs_window_nav_ws_bytes(1 << 20, 2, 3, 1), lib.hs_window_frames_ws_bytes(1 << 20, 2, 3, 1)
    assert nav + (10 << 20) <= frames <= nav + (11 << 20) and frames == lib.hs_window_frames_ws_bytes(1 << 20, 2, 3, 8)
    assert lib.hs_window_frames_ws_bytes(-1, 2, 3, 1) == 0
