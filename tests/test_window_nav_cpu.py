"""Window navigation without a GPU: the model against a brute force straight from the definition, the
grammar against the API and its renderings, schema types and names, the refusals of the API, the parser, the planner and the
stage lowerings, and the argument checks of hs_window_nav, which are answered before anything is launched."""

from __future__ import annotations

import ctypes as C
import math
from datetime import datetime

import numpy as np
import pytest

from minispark_amd import tasks as t
from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SemanticError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import Col, Lit, WindowItem
from minispark_amd.sql import Functions as F
from tests import test_window_agg_cpu, test_window_cpu
from tests.conftest import load_golden
from tests.test_distinct_cpu import _golden_frames
from tests.test_parser import render
from tests.window_nav_model import FRAMES, brute_force, ntile_bucket, window_nav_model


def T(name="t"):
    return DataFrame(object()).table(name)


ORDERS = lambda: load_golden("e2e_join_select")["paths"]["orders"]  # noqa: E731 - user_id, product, quantity, price ...
LINEITEM = lambda: load_golden("q1_multiblock")["paths"]["lineitem"]  # noqa: E731


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_the_model_on_a_hand_written_case():
    part = ["a", "b", "a", "a", "b", "a"]
    key = [5, 1, 5, 3, 1, 9]
    v = [10, 20, 30, 40, 50, 60]
    # 'a' in order: row 3 (3), rows 0 and 2 (5, 5: peers, input order), row 5 (9); 'b': rows 1 and 4 (peers)
    spec = (6, [part], [(key, True)], v)
    assert window_nav_model(*spec, "lag", k=1, default=-1) == [40, -1, 10, -1, 20, 30]
    assert window_nav_model(*spec, "lead", k=1, default=-1) == [30, 50, 60, 10, -1, -1]
    assert window_nav_model(*spec, "lead", k=2, default=0) == [60, 0, 0, 30, 0, 0]
    assert window_nav_model(*spec, "lag", k=0, default=-1) == v
    assert window_nav_model(*spec, "first_value", frame="range") == [40, 20, 40, 40, 20, 40]
    assert window_nav_model(*spec, "last_value", frame="rows") == v
    assert window_nav_model(*spec, "last_value", frame="range") == [30, 50, 30, 40, 50, 60]   # the LAST peer, not the partition's last
    assert window_nav_model(*spec, "last_value", frame="partition") == [60, 50, 60, 60, 50, 60]
    assert window_nav_model(*spec, "ntile", buckets=2).tolist() == [1, 1, 2, 1, 2, 2]
    assert window_nav_model(6, [], [], v, "lag", k=2, default=None) == [None, None, 10, 20, 30, 40]  # no keys: input order
    assert window_nav_model(0, [[]], [([], True)], [], "lead", k=1, default=0) == []


def test_ntile_on_the_two_worked_examples_and_never_an_empty_bucket_before_a_full_one():
    assert ntile_bucket(np.arange(1, 11), 10, 4).tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 4, 4]      # sizes 3, 3, 2, 2
    assert ntile_bucket(np.arange(1, 4), 3, 5).tolist() == [1, 2, 3]
    assert window_nav_model(10, [], [], None, "ntile", buckets=4).tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    assert window_nav_model(3, [], [], None, "ntile", buckets=5).tolist() == [1, 2, 3]
    for rows in (1, 2, 7, 64, 65):
        for buckets in (1, 2, 3, 7, rows - 1, rows, rows + 1, 1000, (1 << 31) - 1):
            if buckets < 1:
                continue
            got = ntile_bucket(np.arange(1, rows + 1), rows, buckets)
            sizes = np.bincount(got)[1:]
            assert got[0] == 1 and np.all(np.diff(got) >= 0) and got[-1] == min(rows, buckets)
            assert sizes.max() - sizes.min() <= 1 and np.all(np.diff(sizes) <= 0)       # the larger buckets first


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 201)) if seed else 200
    part = [rng.integers(0, 4, n).tolist()] if seed % 3 else []
    order = [] if seed == 4 else [(rng.integers(0, 5, n).tolist(), bool(seed % 2))]   # five values: heavy ties
    if seed == 5:
        order.append((rng.choice([0.0, -0.0, 1.5, math.nan], n).tolist(), True))
    cells = [int(x) for x in rng.integers(-(1 << 31), 1 << 31, n)]
    spec = (n, part, order, cells)
    for k in (0, 1, 2, 5, n - 1, n, n + 3):
        for kind in ("lag", "lead"):
            assert window_nav_model(*spec, kind, k=k, default="none") == brute_force(*spec, kind, k=k, default="none"), (kind, k)
    for frame in FRAMES:
        for kind in ("first_value", "last_value"):
            assert window_nav_model(*spec, kind, frame=frame) == brute_force(*spec, kind, frame=frame), (kind, frame)
    for buckets in (1, 2, 3, 7, max(n - 1, 1), n, n + 1, 1000):
        assert window_nav_model(*spec, "ntile", buckets=buckets).tolist() == brute_force(*spec, "ntile", buckets=buckets), buckets


# ---- grammar and API ---------------------------------------------------------------------------------------------------
OVER = dict(partition_by=[Col("k")], order_by=[Col("o").desc()])
CASES = [
    ("SELECT k, o, v, LAG(v, 1, 0) OVER (PARTITION BY k ORDER BY o DESC) FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.lag(Col("v"), 1, 0).over(**OVER)),
     "LAG(v, 1, 0) OVER (PARTITION BY k ORDER BY o DESC) AS lag_v"),
    ("SELECT k, o, v, LEAD( v , 2 , -7 )  OVER( PARTITION BY k  ORDER BY o DESC ) AS nxt FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.lead(Col("v"), 2, -7).over(**OVER).alias("nxt")),
     "LEAD(v, 2, -7) OVER (PARTITION BY k ORDER BY o DESC) AS nxt"),
    ("SELECT v, LAG(v,0,-1.5) OVER () FROM 't';",
     lambda: T().select(Col("v")).window(F.lag(Col("v"), 0, -1.5).over()),
     "LAG(v, 0, -1.5) OVER () AS lag_v"),
    ("SELECT d, LEAD(d, 1, '1970-01-01') OVER (ORDER BY d) AS nxt FROM 't';",
     lambda: T().select(Col("d")).window(F.lead(Col("d"), 1, "1970-01-01").over(order_by=[Col("d")]).alias("nxt")),
     "LEAD(d, 1, '1970-01-01') OVER (ORDER BY d ASC) AS nxt"),
    ("SELECT k, v, FIRST_VALUE(v) OVER (PARTITION BY k) FROM 't';",
     lambda: T().select(Col("k"), Col("v")).window(F.first_value(Col("v")).over(partition_by=[Col("k")])),
     "FIRST_VALUE(v) OVER (PARTITION BY k) AS first_value_v"),
    ("SELECT k, o, v, LAST_VALUE( v ) OVER (PARTITION BY k ORDER BY o DESC) FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.last_value(Col("v")).over(**OVER)),
     "LAST_VALUE(v) OVER (PARTITION BY k ORDER BY o DESC RANGE UNBOUNDED PRECEDING) AS last_value_v"),
    ("SELECT k, o, v, LAST_VALUE(v) OVER (PARTITION BY k ORDER BY o DESC ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW) AS l FROM 't';",
     lambda: T().select(Col("k"), Col("o"), Col("v")).window(F.last_value(Col("v")).over(**OVER, rows=True).alias("l")),
     "LAST_VALUE(v) OVER (PARTITION BY k ORDER BY o DESC ROWS UNBOUNDED PRECEDING) AS l"),
    ("SELECT k, o, NTILE(4) OVER (PARTITION BY k ORDER BY o DESC) FROM 't';",
     lambda: T().select(Col("k"), Col("o")).window(F.ntile(4).over(**OVER)),
     "NTILE(4) OVER (PARTITION BY k ORDER BY o DESC) AS ntile"),
    ("SELECT DISTINCT k, NTILE( 10 ) OVER (ORDER BY k) AS q FROM 't' QUALIFY q <= 1 ORDER BY k LIMIT 5;",
     lambda: T().select(Col("k")).window(F.ntile(10).over(order_by=[Col("k")]).alias("q")).qualify(Col("q") <= Lit(1))
     .distinct().order_by(Col("k")).limit(5),
     "NTILE(10) OVER (ORDER BY k ASC) AS q"),
    ("SELECT k, SUM(v) AS s, LAG(s, 1, 0) OVER (ORDER BY k) AS prev FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.sum(Col("v")).alias("s")).select(Col("k"), Col("s"))
     .window(F.lag(Col("s"), 1, 0).over(order_by=[Col("k")]).alias("prev")),
     "LAG(s, 1, 0) OVER (ORDER BY k ASC) AS prev"),
    ("SELECT k, v, ROW_NUMBER() OVER (ORDER BY k) AS rn, SUM(v) OVER (ORDER BY k) AS s, LAG(v, 1, 0) OVER (ORDER BY k) AS p FROM 't';",
     lambda: T().select(Col("k"), Col("v")).window(F.row_number().over(order_by=[Col("k")]).alias("rn"),
                                                   F.sum(Col("v")).over(order_by=[Col("k")]).alias("s"),
                                                   F.lag(Col("v"), 1, 0).over(order_by=[Col("k")]).alias("p")),
     "LAG(v, 1, 0) OVER (ORDER BY k ASC) AS p"),
]


@pytest.mark.parametrize("sql,build,shown", CASES, ids=[f"{i}" for i in range(len(CASES))])
def test_text_builds_the_same_tree_as_the_api(sql, build, shown):
    got, want = parse_sql(sql, object()).task, build().task
    assert type(got) is t.SortTask and got.windows and type(got.parent_task) is not t.SortTask  # ONE task carries all
    assert render(got) == render(want) and repr(got) == repr(want)
    fields = lambda w: (w.kind, str(w.arg), w.frame, w.name, w.offset, w.default, w.buckets)  # noqa: E731
    assert [fields(w) for w in got.windows] == [fields(w) for w in want.windows]
    assert str(got.windows[-1]) == shown and shown in repr(got) and shown in got.describe()


def test_every_spelling_of_the_frame_clause_on_first_and_last_value():
    frames = {"": "range", " ROWS UNBOUNDED PRECEDING": "rows", " ROWS BETWEEN UNBOUNDED PRECEDING": "rows",
              " ROWS UNBOUNDED PRECEDING AND CURRENT ROW": "rows", " ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": "rows",
              " RANGE UNBOUNDED PRECEDING": "range", " RANGE BETWEEN UNBOUNDED PRECEDING": "range",
              " RANGE UNBOUNDED PRECEDING AND CURRENT ROW": "range", " RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": "range"}
    for head in ("FIRST_VALUE", "LAST_VALUE"):
        for clause, frame in frames.items():
            item = parse_sql(f"SELECT v, {head}(v) OVER (ORDER BY v{clause}) FROM 't';", object()).task.windows[0]
            assert (item.kind, item.frame, item.name) == (head.lower(), frame, f"{head.lower()}_v")
            bare = parse_sql(f"SELECT v, {head}(v) OVER ({clause.strip()}) FROM 't';", object()).task.windows[0]
            assert bare.frame == ("rows" if frame == "rows" else "partition") and bare.order_by == []
        # another frame: no window item, so the text is what it was to the older grammar (as ROW_NUMBER() OVER (ORDER BY a + 1))
        with pytest.raises(SemanticError, match=f"^Unsupported function: {head}$"):
            parse_sql(f"SELECT v, {head}(v) OVER (ORDER BY v ROWS 3 PRECEDING) FROM 't';", object())


def test_the_older_accepted_texts_build_the_trees_they_built():
    for sql, build in [*test_window_cpu.CASES, *test_window_agg_cpu.CASES]:
        got, want = parse_sql(sql, object()).task, build().task
        assert render(got) == render(want) and repr(got) == repr(want)
        assert all(w.kind not in WindowItem.NAVIGATION and (w.offset, w.default, w.buckets) == (None, None, None) for w in got.windows)
    assert str(F.sum(Col("v")).over(partition_by=[Col("k")], order_by=[Col("o").desc()], rows=True).alias("s")) == \
        "SUM(v) OVER (PARTITION BY k ORDER BY o DESC ROWS UNBOUNDED PRECEDING) AS s"
    assert str(F.row_number().over()) == "ROW_NUMBER() OVER () AS row_number"
    plain = parse_sql("SELECT a FROM 't' ORDER BY a LIMIT 3;", object()).task
    assert "windows" not in repr(plain) and "offset" not in repr(plain)


def test_schema_types_and_default_names_per_function():
    base = lambda: T(LINEITEM()).select(Col("l_shipmode"), Col("l_orderkey"), Col("l_quantity"), Col("l_shipdate"))  # noqa: E731
    items = [F.lag(Col("l_orderkey"), 1, 0).over(), F.lead(Col("l_quantity"), 1, 0).over(), F.first_value(Col("l_shipdate")).over(),
             F.last_value(Col("l_quantity")).over(), F.ntile(3).over(), F.lead(Col("l_shipdate"), 3, "1999-12-31 23:59:59").over(),
             F.lag(Col("l_quantity"), 2, -0.25).over()]
    schema = base().window(*items[:5]).task.validate_schema()
    assert [(n, str(ty)) for n, ty in schema[4:]] == [("lag_l_orderkey", "INTEGER"), ("lead_l_quantity", "FLOAT"),
                                                     ("first_value_l_shipdate", "TIMESTAMP"), ("last_value_l_quantity", "FLOAT"),
                                                     ("ntile", "INTEGER")]
    schema = base().window(*items[5:]).task.validate_schema()
    assert [(n, str(ty)) for n, ty in schema[4:]] == [("lead_l_shipdate", "TIMESTAMP"), ("lag_l_quantity", "FLOAT")]
    with pytest.raises(ValueError, match="Duplicate.*ntile"):
        base().window(F.ntile(2).over(), F.ntile(3).over(order_by=[Col("l_orderkey")])).task.validate_schema()
    from minispark_amd.constants import ColumnType

    assert items[0].default_bits(ColumnType.INTEGER) == 0 and F.lag(Col("a"), 1, -1).default_bits(ColumnType.INTEGER) == 0xFFFFFFFF
    assert items[6].default_bits(ColumnType.FLOAT) == 0xBE800000 and F.lag(Col("a"), 1, 3).default_bits(ColumnType.FLOAT) == 0x40400000
    assert F.lag(Col("a"), 1, 0.1).default_bits(ColumnType.FLOAT) == int(np.float32(0.1).view(np.uint32))   # rounded to f32
    want = int((datetime(1999, 12, 31, 23, 59, 59) - datetime(1970, 1, 1)).total_seconds()) * 1_000_000
    assert items[5].default_bits(ColumnType.TIMESTAMP) == want
    assert F.lag(Col("a"), 1, "1969-12-31").default_bits(ColumnType.TIMESTAMP) == (-86_400_000_000) & 0xFFFFFFFFFFFFFFFF


def test_items_of_one_spec_share_a_sort_whatever_they_are():
    items = [F.lag(Col("v"), 1, 0).over(**OVER), F.rank().over(**OVER), F.sum(Col("v")).over(**OVER, rows=True),
             F.ntile(4).over(**OVER), F.last_value(Col("v")).over(**OVER)]
    assert len({i.spec() for i in items}) == 1 and F.ntile(4).over(partition_by=[Col("k")]).spec() != items[0].spec()


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["LAG", "LEAD"])
def test_k_and_the_default_are_mandatory(head):
    for text in (f"SELECT v, {head}(v) OVER (ORDER BY v) FROM 't';", f"SELECT v, {head}(v, 1) OVER (ORDER BY v) FROM 't';",
                 f"SELECT v, {head}( v ,1 ) OVER () AS p FROM 't';"):
        with pytest.raises(ValueError, match=rf"mandatory.*{head}\(v, 1, 0\)"):
            parse_sql(text, object())
    make = F.lag if head == "LAG" else F.lead
    with pytest.raises(ValueError, match=rf"mandatory.*{head}\(v, 1, 0\)"):
        make(Col("v"))
    with pytest.raises(ValueError, match="mandatory"):
        make(Col("v"), 1)
    with pytest.raises(ValueError, match="two literals"):
        parse_sql(f"SELECT v, {head}(v, 1, 0, 0) OVER (ORDER BY v) FROM 't';", object())


def test_without_over_it_is_the_unsupported_function_it_was():
    for text in ("SELECT a, LAG(a) FROM 't';", "SELECT LAG(a) AS p FROM 't';", "SELECT a, LEAD(a, 1, 0) FROM 't';",
                 "SELECT a, NTILE(4) FROM 't';", "SELECT a, FIRST_VALUE(a) FROM 't';", "SELECT a, LAST_VALUE(a) AS l FROM 't';"):
        with pytest.raises(SemanticError, match="^Unsupported function: (LAG|LEAD|NTILE|FIRST_VALUE|LAST_VALUE)$"):
            parse_sql(text, object())
    # a column whose name starts like a head is a column
    assert [c.name for c in parse_sql("SELECT LAGOON, NTILES FROM 't';", object()).task.columns] == ["LAGOON", "NTILES"]


def test_a_frame_on_lag_lead_and_ntile_is_refused():
    for item in ("LAG(a, 1, 0)", "LEAD(a, 1, 0)", "NTILE(4)"):
        for frame in ("ROWS UNBOUNDED PRECEDING", "RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"):
            with pytest.raises(ValueError, match="takes no frame clause"):
                parse_sql(f"SELECT a, {item} OVER (ORDER BY a {frame}) FROM 't';", object())
    for make in (lambda: F.lag(Col("a"), 1, 0), lambda: F.lead(Col("a"), 1, 0), lambda: F.ntile(4)):
        with pytest.raises(ValueError, match="takes no frame clause"):
            make().over(order_by=[Col("a")], rows=True)


def test_k_and_n_are_integer_literals_in_their_ranges():
    for bad in (0, -1, 1 << 31, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="1 <= n < 2\\^31"):
            F.ntile(bad)
    for text in ("NTILE(0)", "NTILE(-1)", "NTILE(2147483648)", "NTILE(1.5)", "NTILE('4')"):
        with pytest.raises(ValueError, match="1 <= n < 2\\^31"):
            parse_sql(f"SELECT a, {text} OVER (ORDER BY a) FROM 't';", object())
    assert F.ntile((1 << 31) - 1).buckets == (1 << 31) - 1
    for bad in (-1, 1 << 31, 1.0, "1", True):
        with pytest.raises(ValueError, match="0 <= k < 2\\^31"):
            F.lag(Col("a"), bad, 0)
    for text in ("LAG(a, -1, 0)", "LEAD(a, 2147483648, 0)", "LAG(a, 1.5, 0)", "LEAD(a, '1', 0)"):
        with pytest.raises(ValueError, match="0 <= k < 2\\^31"):
            parse_sql(f"SELECT a, {text} OVER (ORDER BY a) FROM 't';", object())
    assert parse_sql("SELECT a, LAG(a, 2147483647, 0) OVER () FROM 't';", object()).task.windows[0].offset == (1 << 31) - 1
    assert F.lead(Col("a"), 0, 0).offset == 0
    with pytest.raises(SemanticError, match="^Unsupported function: NTILE$"):  # no literal: no window item
        parse_sql("SELECT a, NTILE() OVER (ORDER BY a) FROM 't';", object())
    with pytest.raises(ValueError, match="literal"):
        F.lag(Col("a"), 1, Col("b"))  # a default that is a column


def test_the_argument_is_a_plain_numeric_or_timestamp_column_of_the_result():
    base = lambda: T(ORDERS()).select(Col("product"), Col("quantity"), Col("price"))  # noqa: E731 - STRING, INTEGER, FLOAT
    for item in (F.lag(Col("product"), 1, 0), F.lead(Col("product"), 1, "x"), F.first_value(Col("product")), F.last_value(Col("product"))):
        with pytest.raises(TypeError, match='"product" is STRING'):
            base().window(item.over()).task.validate_schema()
    with pytest.raises(TypeError, match='"product" is STRING'):
        parse_sql(f"SELECT product, LAG(product, 1, 0) OVER (ORDER BY product) FROM '{ORDERS()}';", object()).task.validate_schema()
    with pytest.raises(ValueError, match='"user_id" not found'):  # not selected: the error a key raises
        base().window(F.lag(Col("user_id"), 1, 0).over()).task.validate_schema()
    with pytest.raises(ValueError, match='"n" not found'):        # another window item is no argument
        base().window(F.ntile(2).over().alias("n"), F.lag(Col("n"), 1, 0).over().alias("m")).task.validate_schema()
    for make in (lambda a: F.lag(a, 1, 0), lambda a: F.lead(a, 1, 0), F.first_value, F.last_value):
        with pytest.raises(ValueError, match="plain columns.*alias"):
            make(Col("a") + 1)
    for text in ("LAG(a + 1, 1, 0)", "LEAD(a * 2, 1, 0)", "FIRST_VALUE(a + 1)", "LAST_VALUE(a - 1)", "LAG(a + 1)"):
        with pytest.raises(SemanticError, match="alias the expression in the select list"):
            parse_sql(f"SELECT a, {text} OVER (ORDER BY a) FROM 't';", object())
    with pytest.raises(ValueError, match="plain columns"):
        F.lag(Col("a"), 1, 0).over(order_by=[Col("a") * 2])
    with pytest.raises(ValueError, match="over"):
        T().select(Col("a")).window(F.ntile(4))  # no .over(...)


def test_the_default_has_the_type_of_its_column():
    base = lambda: T(LINEITEM()).select(Col("l_orderkey"), Col("l_quantity"), Col("l_shipdate"))  # noqa: E731 - INTEGER, FLOAT, TIMESTAMP
    check = lambda item: base().window(item.over()).task.validate_schema()  # noqa: E731
    with pytest.raises(TypeError, match='"l_orderkey" is INTEGER'):
        check(F.lag(Col("l_orderkey"), 1, 0.5))                       # a decimal for an INTEGER column
    with pytest.raises(TypeError, match='"l_orderkey" is INTEGER'):
        parse_sql(f"SELECT l_orderkey, LAG(l_orderkey, 1, 0.5) OVER () FROM '{LINEITEM()}';", object()).task.validate_schema()
    with pytest.raises(TypeError, match="INTEGER"):
        check(F.lead(Col("l_orderkey"), 1, "1970-01-01"))
    for beyond in (1 << 31, -(1 << 31) - 1):
        with pytest.raises((OverflowError, ValueError), match="32 bits"):
            check(F.lag(Col("l_orderkey"), 1, beyond))
    with pytest.raises((OverflowError, ValueError), match="32 bits"):
        parse_sql(f"SELECT l_orderkey, LEAD(l_orderkey, 1, 2147483648) OVER () FROM '{LINEITEM()}';", object()).task.validate_schema()
    check(F.lag(Col("l_orderkey"), 1, -(1 << 31)))
    check(F.lag(Col("l_orderkey"), 1, (1 << 31) - 1))
    with pytest.raises(TypeError, match='"l_quantity" is FLOAT'):
        check(F.lag(Col("l_quantity"), 1, "0"))
    for beyond in (math.inf, math.nan, 1e39):
        with pytest.raises((OverflowError, ValueError)):
            check(F.lag(Col("l_quantity"), 1, beyond))
    check(F.lag(Col("l_quantity"), 1, 7))                              # an integer literal is a number
    for wrong in (0, 0.0, "yesterday"):
        with pytest.raises(TypeError, match="TIMESTAMP"):
            check(F.lead(Col("l_shipdate"), 1, wrong))
    check(F.lead(Col("l_shipdate"), 1, "1970-01-01"))


def test_a_ninth_item_names_the_limit():
    items = [F.lag(Col("a"), i, 0).over(order_by=[Col("a")]).alias(f"w{i}") for i in range(9)]
    with pytest.raises(ValueError, match="at most 8 window items"):
        T().select(Col("a")).window(*items)
    assert len(T().select(Col("a")).window(*items[:8]).task.windows) == 8
    text = "SELECT a, " + ", ".join(f"NTILE({i + 1}) OVER (ORDER BY a) AS w{i}" for i in range(9)) + " FROM 't';"
    with pytest.raises(ValueError, match="at most 8 window items"):
        parse_sql(text, object())
    with pytest.raises(ValueError, match="at most 12"):
        T().select(Col("a")).window(F.ntile(2).over(partition_by=[Col("a")] * 7, order_by=[Col("a")] * 6))


# ---- planner and stage lowerings ---------------------------------------------------------------------------------------
KEYS = {"scan": "product", "group": "p", "join": "u.first_name", "join_group": "n"}


def test_a_navigation_item_below_a_join_or_another_operation_is_refused_when_planned():
    g = load_golden("e2e_join_select")
    right = (DataFrame(object()).table(g["paths"]["orders"]).alias("o")
             .window(F.lag(Col("o.price"), 1, 0).over(order_by=[Col("o.price")]).alias("prev")))
    joined = DataFrame(object()).table(g["paths"]["users"]).alias("u").join(right, on=Col("u.user_id") == Col("o.user_id"),
                                                                            how="inner")
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(joined.task)
    below = _golden_frames()["scan"]().window(F.ntile(4).over(order_by=[Col("product")])).filter(Col("quantity") > 1)
    with pytest.raises(ValueError, match="window.*must be the last operation"):
        PhysicalPlan.generate_physical_plan(below.task)


def test_all_five_stage_lowerings_refuse_a_plan_with_a_navigation_item():
    from minispark_amd import stage as st

    lowerings = [st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                 st.lower_join_group_stage_plan]
    for lower in lowerings:
        for shape, key in KEYS.items():
            with pytest.raises(st.StageUnsupported):
                lower(_golden_frames()[shape]().window(F.ntile(3).over(order_by=[Col(key)]).alias("q")).task)
        with pytest.raises(st.StageUnsupported):
            lower(_golden_frames()["scan"]().window(F.lag(Col("quantity"), 1, 0).over(order_by=[Col("product")])).task)


def test_the_windowed_task_adds_a_timestamp_column_in_the_result_stage():
    frame = (T(LINEITEM()).select(Col("l_orderkey"), Col("l_shipdate"))
             .window(F.lead(Col("l_shipdate"), 1, "1970-01-01").over(order_by=[Col("l_orderkey")]).alias("nxt")))
    last = PhysicalPlan.generate_physical_plan(frame.task).stages[-1]
    sort = next(x for x in last.consumers if type(x).__name__ == "SortTask")
    assert [str(ty) for _, ty in sort.inferred_schema] == ["INTEGER", "TIMESTAMP", "TIMESTAMP"]
    assert last.writer.inferred_schema[-1][0] == "nxt"


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

    def call(n_part=1, n_keys=2, nrows=4, funcs=(hs.WIN_LAG,), frames=(hs.WIN_FRAME_RANGE,), kinds=(hs.I32,), params=(1,), outs=out,
             work=ws, keys=key, no_values=False, no_frames=False, no_params=False, no_defaults=False, data=4096):
        n = len(funcs)
        fs = (C.c_int32 * max(n, 1))(*funcs)
        fr = (C.c_int32 * max(n, 1))(*(list(frames) * n)[:n])
        vals = (hs.hs_col * max(n, 1))()
        for i in range(n):
            vals[i].kind, vals[i].fixed_len, vals[i].data = (list(kinds) * n)[i], -1, data
        ps = (C.c_int64 * max(n, 1))(*(list(params) * n)[:n])
        ds = (C.c_uint64 * max(n, 1))()
        return lib.hs_window_nav(None, keys, desc, n_part, n_keys, nrows, fs, None if no_frames else fr, None if no_values else vals,
                                 None if no_params else ps, None if no_defaults else ds, n, outs, work, None)

    assert call(n_keys=13) == 2 and b"12" in lib.hs_last_error()
    assert call(nrows=1 << 31) == 2 and b"2^31" in lib.hs_last_error()
    assert call(funcs=[hs.WIN_LAG] * 9) == 2 and b"8" in lib.hs_last_error()
    assert call(funcs=(13,)) == 1 and b"function 13" in lib.hs_last_error()
    assert call(funcs=(-1,)) == 1
    for f in (hs.WIN_FIRST_VALUE, hs.WIN_LAST_VALUE, hs.WIN_MIN):
        assert call(funcs=(hs.WIN_NTILE, f), frames=(0, 3)) == 1 and b"item 1: frame 3" in lib.hs_last_error()
        assert call(funcs=(f,), no_frames=True) == 1 and b"item 0" in lib.hs_last_error()
    for f in (hs.WIN_LAG, hs.WIN_LEAD):
        for k in (-1, 1 << 31):
            assert call(funcs=(hs.WIN_ROW_NUMBER, f), params=(0, k)) == 1
            assert b"item 1" in lib.hs_last_error() and b"offset k" in lib.hs_last_error()
        assert call(funcs=(f,), no_params=True) == 1 and b"item 0" in lib.hs_last_error() and b"params" in lib.hs_last_error()
        assert call(funcs=(f,), no_defaults=True) == 1 and b"item 0" in lib.hs_last_error() and b"default" in lib.hs_last_error()
    for n in (0, -1, 1 << 31):
        assert call(funcs=(hs.WIN_ROW_NUMBER, hs.WIN_NTILE), params=(0, n)) == 1
        assert b"item 1" in lib.hs_last_error() and b"bucket count n" in lib.hs_last_error()
    assert call(funcs=(hs.WIN_NTILE,), no_params=True) == 1 and b"item 0" in lib.hs_last_error()
    for f in (hs.WIN_LAG, hs.WIN_LEAD, hs.WIN_FIRST_VALUE, hs.WIN_LAST_VALUE):
        for kind in (hs.F64, hs.STR, hs.U8, 6, 7, 16, 17, 0x100 | hs.I32):  # other types, STRING, narrow, virtual, pair-indexed
            assert call(funcs=(hs.WIN_ROW_NUMBER, f), kinds=(hs.I32, kind)) == 1
            assert b"item 1" in lib.hs_last_error() and str(kind).encode() in lib.hs_last_error()
        assert call(funcs=(f,), no_values=True) == 1 and b"item 0" in lib.hs_last_error()
        assert call(funcs=(hs.WIN_ROW_NUMBER, f), data=None) == 1 and b"item 1" in lib.hs_last_error() and b"null" in lib.hs_last_error()
    assert call(funcs=(hs.WIN_COUNT, hs.WIN_AVG), kinds=(hs.I32, hs.I64)) == 1 and b"item 1" in lib.hs_last_error()  # the aggregates' own
    assert call(n_part=2, funcs=(hs.WIN_LAG, hs.WIN_RANK)) == 1 and b"order key" in lib.hs_last_error()
    assert call(n_part=3) == 1 and call(n_part=-1) == 1 and call(nrows=-1) == 1 and call(funcs=()) == 1 and call(outs=None) == 1
    assert call(work=None) == 1 and call(keys=None) == 1
    # NTILE reads no argument, the older items neither parameters nor defaults; without rows nothing is launched
    assert call(nrows=0, funcs=(hs.WIN_NTILE, hs.WIN_ROW_NUMBER, hs.WIN_COUNT), kinds=(hs.STR,), no_defaults=True) == 0
    assert call(nrows=0, funcs=(hs.WIN_RANK, hs.WIN_SUM), no_params=True, no_defaults=True) == 0
    assert call(nrows=0, funcs=(hs.WIN_LAG, hs.WIN_LEAD, hs.WIN_FIRST_VALUE), kinds=(hs.I32, hs.F32, hs.I64), params=((1 << 31) - 1,)) == 0
    assert call(nrows=0, funcs=(hs.WIN_FIRST_VALUE,), no_params=True, no_defaults=True, data=None) == 0
    # 8 bytes per row for the cells in sorted order whatever the items are, and two tables of frame ends
    assert (lib.hs_window_nav_ws_bytes(1 << 20, 2, 3, 1) >= lib.hs_window_agg_ws_bytes(1 << 20, 2, 3, 1) + (16 << 20)
            and lib.hs_window_nav_ws_bytes(1 << 20, 2, 3, 8) == lib.hs_window_nav_ws_bytes(1 << 20, 2, 3, 1))
    assert lib.hs_window_nav_ws_bytes(-1, 2, 3, 1) == 0
    assert (hs.WIN_LAG, hs.WIN_LEAD, hs.WIN_FIRST_VALUE, hs.WIN_LAST_VALUE, hs.WIN_NTILE) == (8, 9, 10, 11, 12)
    # and hs_window_agg still refuses what is not its own
    assert lib.hs_window_agg(None, key, desc, 1, 2, 4, (C.c_int32 * 1)(8), (C.c_int32 * 1)(0), None, 1, out, ws, None) == 1
    assert b"function 8" in lib.hs_last_error()
