"""COUNT(DISTINCT e) without a GPU: the Python model of the marks against the set sizes they must add up to, the grammar
against the API, the physical plan (one MarkFirstTask under the partial aggregate, an integer SUM from there on), the
refusals that need no device and the argument checks of hs_mark_first - and one guard that holds before the feature too:
the corpus of query texts in tests/golden/distinct_parser_corpus.json keeps the trees it built."""

from __future__ import annotations

import ctypes as C
import json
import random
from pathlib import Path

import pytest

from minispark_amd import tasks as t
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.parser import SqlSyntaxError, parse_sql
from minispark_amd.plan import PhysicalPlan
from minispark_amd.sql import AggCol, Col, Functions as F
from tests.conftest import load_golden
from tests.count_distinct_model import counts, marks
from tests.test_parser import render

CORPUS = json.loads((Path(__file__).parent / "golden" / "distinct_parser_corpus.json").read_text())


def T(name="t"):
    return DataFrame(object()).table(name)


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_the_marks_of_a_key_add_up_to_the_size_of_its_set(seed):
    rng = random.Random(seed)
    n = rng.choice([0, 1, 2, 7, 60, 300])
    pool = [0.0, -0.0, float("nan"), float("nan"), 1.5, float("inf"), -float("inf"), b"a", b"a\0", b"", 3, -3]
    keys = [rng.choice([b"x", b"y", 5, (1, b"q"), (1, b"r")]) for _ in range(n)]
    values = [rng.choice(pool) for _ in range(n)]
    alive = [rng.random() < 0.6 for _ in range(n)]
    for living in (None, alive):
        sel = None if living is None else [r for r in range(n) if living[r]]
        m = marks([keys, values], sel)
        assert len(m) == n and set(m) <= {0, 1}
        assert all(m[r] == 0 for r in range(n) if living is not None and not living[r])
        want = counts(keys, values, living)
        got: dict = {}
        for r in range(n):
            if living is None or living[r]:
                got[keys[r]] = got.get(keys[r], 0) + m[r]
        assert got == want


def test_the_model_marks_first_occurrences_in_input_order():
    assert marks([[3, 1, 3, 1, 2]]) == [1, 1, 0, 0, 1]
    assert marks([[3, 1, 3, 1, 2]], sel=[2, 3, 4]) == [0, 0, 1, 1, 1]  # the first occurrences lie outside the list
    assert marks([[3, 1, 3]], sel=[]) == [0, 0, 0]
    assert marks([[0.0, -0.0, float("nan"), float("nan")]]) == [1, 0, 1, 0]
    assert marks([[b"a", b"a\0", b"a"]]) == [1, 1, 0]
    assert counts([None] * 3, [1, 1, 2]) == {None: 2} and counts([b"k"], [1], [False]) == {}


# ---- grammar and API -----------------------------------------------------------------------------------------------------
CASES = [
    ("SELECT COUNT(DISTINCT x) FROM 't';", lambda: T().agg(F.count_distinct(Col("x")))),
    ("SELECT COUNT(DISTINCT x) AS d FROM 't';", lambda: T().agg(F.count_distinct(Col("x")).alias("d"))),
    ("SELECT k, COUNT(DISTINCT x) AS d, SUM(y) FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.count_distinct(Col("x")).alias("d"), F.sum(Col("y")))
     .select(Col("k"), Col("d"), Col("sum_y"))),
    ("SELECT a, b, COUNT(DISTINCT x) FROM 't' GROUP BY (a, b);",
     lambda: T().group_by(Col("a"), Col("b")).agg(F.count_distinct(Col("x")))
     .select(Col("a"), Col("b"), Col("count_distinct_x"))),
    ("SELECT k, COUNT() FROM 't' GROUP BY k HAVING COUNT(DISTINCT x) > 1;",
     lambda: T().group_by(Col("k")).agg(F.count(), F.count_distinct(Col("x")).alias("_having_count_distinct_x"))
     .filter(Col("_having_count_distinct_x") > 1).select(Col("k"), Col("count"))),
    ("SELECT k, COUNT(DISTINCT x * 2 + 1) AS d FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.count_distinct(Col("x") * 2 + 1).alias("d")).select(Col("k"), Col("d"))),
    ("SELECT COUNT(DISTINCT YEAR(d)) FROM 't' WHERE x > 3;",
     lambda: T().filter(Col("x") > 3).agg(F.count_distinct(F.year(Col("d"))))),
    ("SELECT k, COUNT(DISTINCT x) AS dx, COUNT(DISTINCT y) AS dy FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(F.count_distinct(Col("x")).alias("dx"), F.count_distinct(Col("y")).alias("dy"))
     .select(Col("k"), Col("dx"), Col("dy"))),
]


@pytest.mark.parametrize("sql,build", CASES, ids=[c[0][:50] for c in CASES])
def test_text_builds_the_same_tree_as_the_api(sql, build):
    assert render(parse_sql(sql, object()).task) == render(build().task)


def test_the_aggregate_column_is_an_integer_named_after_its_argument():
    agg = F.count_distinct(Col("x"))
    assert type(agg) is AggCol and (agg.type, agg.name) == ("count_distinct", "count_distinct_x")
    assert agg.infer_type([("x", ColumnType.STRING)]) == ColumnType.INTEGER
    assert agg.alias("d") is agg and agg.name == "d"
    with pytest.raises(ValueError, match='"x" not found'):
        agg.infer_type([("y", ColumnType.INTEGER)])
    schema = T(load_golden("q1_multiblock")["paths"]["lineitem"]).group_by(Col("l_returnflag")).agg(
        F.count_distinct(Col("l_shipmode")).alias("modes")).schema
    assert schema == [("l_returnflag", ColumnType.STRING), ("modes", ColumnType.INTEGER)]


@pytest.mark.parametrize("text", ["SELECT COUNT(DISTINCT a, b) FROM 't';", "SELECT COUNT(DISTINCT ) FROM 't';",
                                  "SELECT SUM(DISTINCT a) FROM 't';", "SELECT COUNT(DISTINCT a b) FROM 't';",
                                  "SELECT k FROM 't' GROUP BY k HAVING COUNT(DISTINCT a, b) > 1;"])
def test_malformed_forms_are_rejected(text):
    with pytest.raises((SqlSyntaxError, AssertionError)):
        parse_sql(text, object())


def test_count_of_a_column_called_distinct_raises_what_it_raised():
    with pytest.raises(AssertionError, match="COUNT takes no argument"):
        parse_sql("SELECT COUNT(DISTINCT) FROM 't';", object())


@pytest.mark.parametrize("text", sorted(CORPUS), ids=[f"{i:02d}" for i in range(len(CORPUS))])
def test_a_text_accepted_before_builds_the_tree_it_built_before(text):
    assert render(parse_sql(text, object()).task) == CORPUS[text]


# ---- the plan ------------------------------------------------------------------------------------------------------------
LINEITEM = lambda: load_golden("q1_multiblock")["paths"]["lineitem"]  # noqa: E731


def _stages(frame):
    return PhysicalPlan.generate_physical_plan(frame.task).stages


def test_one_mark_task_sits_directly_under_the_partial_aggregate():
    frame = (T(LINEITEM()).filter(Col("l_quantity") > 25).group_by(Col("l_returnflag"))
             .agg(F.count_distinct(Col("l_shipmode")).alias("modes"), F.sum(Col("l_quantity")), F.avg(Col("l_tax"))))
    scan, final = _stages(frame)
    kinds = [type(x).__name__ for x in scan.consumers]
    assert kinds == ["FilterTask", "MarkFirstTask", "AggregateTask"]
    mark, partial = scan.consumers[1], scan.consumers[2]
    assert partial.parent_task is mark and partial.before_shuffle
    assert str(mark.key) == "l_returnflag" and [(n, str(e)) for n, e in mark.items] == [("__hs_mark0(l_shipmode)", "l_shipmode")]
    assert mark.inferred_schema == [*mark.parent_task.inferred_schema, ("__hs_mark0(l_shipmode)", ColumnType.INTEGER)]
    assert "MarkFirst(key: l_returnflag; __hs_mark0(l_shipmode) <- l_shipmode)" == mark.describe()
    carried = partial.agg_columns[0]
    assert (carried.type, str(carried.original_col), carried.name) == ("sum", "__hs_mark0(l_shipmode)", "modes")
    merge = final.consumers[0]
    assert type(merge).__name__ == "AggregateTask" and not merge.before_shuffle
    assert [(a.type, str(a.original_col)) for a in merge.agg_columns][:2] == [("sum", "modes"), ("sum", "sum_l_quantity")]
    assert final.writer.inferred_schema == [("l_returnflag", ColumnType.STRING), ("modes", ColumnType.INTEGER),
                                            ("sum_l_quantity", ColumnType.FLOAT), ("avg_l_tax", ColumnType.FLOAT)]
    # ... exactly the shape SUM of an INTEGER column gets
    plain = (T(LINEITEM()).filter(Col("l_quantity") > 25).group_by(Col("l_returnflag"))
             .agg(F.sum(Col("l_orderkey")).alias("modes"), F.sum(Col("l_quantity")), F.avg(Col("l_tax"))))
    plain_scan, plain_final = _stages(plain)
    assert [type(x).__name__ for x in plain_scan.consumers] == ["FilterTask", "AggregateTask"]
    assert plain_final.writer.inferred_schema == final.writer.inferred_schema
    assert [str(a) for a in plain_final.consumers[0].agg_columns] == [str(a) for a in merge.agg_columns]


def test_two_counts_of_one_argument_share_a_mark_and_the_row_form_keeps_its_parts():
    frame = (T(LINEITEM()).group_by(Col("l_returnflag"), Col("l_shipmode"))
             .agg(F.count_distinct(Col("l_quantity")).alias("a"), F.count_distinct(Col("l_quantity")).alias("b"),
                  F.count_distinct(F.year(Col("l_shipdate"))).alias("y")))
    scan, final = _stages(frame)
    mark, partial = scan.consumers
    assert type(mark) is t.MarkFirstTask and [n for n, _ in mark.items] == ["__hs_mark0(l_quantity)", "__hs_mark1(year_l_shipdate)"]
    assert [str(p) for p in mark.key_parts()] == ["l_returnflag", "l_shipmode"] and not mark.key.packed
    assert partial.group_by_column.packed
    assert [str(a.original_col) for a in partial.agg_columns] == ["__hs_mark0(l_quantity)"] * 2 + ["__hs_mark1(year_l_shipdate)"]
    assert [type(x).__name__ for x in final.consumers][:2] == ["AggregateTask", "UnpackKeyTask"]
    whole = _stages(T(LINEITEM()).agg(F.count_distinct(Col("l_orderkey"))))
    assert type(whole[0].consumers[0]) is t.MarkFirstTask and whole[0].consumers[0].key is None
    assert whole[0].consumers[0].key_parts() == []
    assert whole[-1].writer.inferred_schema == [("count_distinct_l_orderkey", ColumnType.INTEGER)]


def test_a_query_without_the_aggregate_plans_as_before():
    frame = T(LINEITEM()).group_by(Col("l_returnflag")).agg(F.count(), F.avg(Col("l_tax")))
    assert not any(type(x) is t.MarkFirstTask for st in _stages(frame) for x in st.consumers)


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_a_float_group_key_is_refused_when_planned():
    frame = T(LINEITEM()).group_by(Col("l_quantity")).agg(F.count_distinct(Col("l_orderkey")))
    with pytest.raises(NotImplementedError, match=r"COUNT\(DISTINCT\).*l_quantity.*FLOAT"):
        PhysicalPlan.generate_physical_plan(frame.task)
    frame = T(LINEITEM()).group_by(Col("l_returnflag"), Col("l_tax")).agg(F.count_distinct(Col("l_orderkey")))
    with pytest.raises(NotImplementedError, match=r"COUNT\(DISTINCT\).*l_tax.*FLOAT"):
        PhysicalPlan.generate_physical_plan(frame.task)
    PhysicalPlan.generate_physical_plan(T(LINEITEM()).group_by(Col("l_quantity")).agg(F.count()).task)  # the key itself is fine


def test_a_computed_group_key_is_refused_when_planned():
    frame = T(LINEITEM()).group_by(Col("l_orderkey") + 1).agg(F.count_distinct(Col("l_shipmode")))
    with pytest.raises(NotImplementedError, match=r"COUNT\(DISTINCT\).*plain column"):
        PhysicalPlan.generate_physical_plan(frame.task)


def test_a_string_expression_argument_is_refused_when_planned():
    frame = T(LINEITEM()).group_by(Col("l_returnflag")).agg(F.count_distinct(Col("l_returnflag") + Col("l_shipmode")))
    with pytest.raises(NotImplementedError, match=r"COUNT\(DISTINCT .*l_returnflag.*l_shipmode.*string expression"):
        PhysicalPlan.generate_physical_plan(frame.task)
    frame = T(LINEITEM()).agg(F.count_distinct(Col("l_quantity") > 3))
    with pytest.raises(NotImplementedError, match=r"COUNT\(DISTINCT "):
        PhysicalPlan.generate_physical_plan(frame.task)


def test_all_five_stage_lowerings_refuse_the_plan():
    from minispark_amd import stage as st

    frames = [T(LINEITEM()).group_by(Col("l_returnflag")).agg(F.count_distinct(Col("l_shipmode"))),
              T(LINEITEM()).agg(F.count_distinct(Col("l_shipmode")))]
    for lower in (st.lower_stage_plan, st.lower_join_stage_plan, st.lower_select_stage_plan, st.lower_join_select_stage_plan,
                  st.lower_join_group_stage_plan):
        for frame in frames:
            with pytest.raises(st.StageUnsupported, match=r"^COUNT\(DISTINCT\)$"):
                lower(frame.task)


def test_a_stage_that_reads_its_input_in_pieces_refuses_the_mark_task():
    """The guard both range-by-range routes (scan stage, streamed join) call before they start, on plain task lists."""
    from minispark_amd.execution import ExecutionError, HipExecutionEngine

    scan, _ = _stages(T(LINEITEM()).group_by(Col("l_returnflag")).agg(F.count_distinct(Col("l_shipmode")), F.count()))
    with pytest.raises(ExecutionError, match=r"COUNT\(DISTINCT\).*whole input.*HIPSPARK_HBM_BUDGET: raise the budget"):
        HipExecutionEngine._refuse_marks_in_pieces(list(scan.consumers))
    plain, _ = _stages(T(LINEITEM()).group_by(Col("l_returnflag")).agg(F.count()))
    HipExecutionEngine._refuse_marks_in_pieces(list(plain.consumers))


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu():
    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    key = (hs.hs_col * 13)()
    for k in range(13):
        key[k].kind, key[k].fixed_len, key[k].data = hs.I32, -1, 4096  # never dereferenced by the checks
    out = (C.c_int32 * 4)()
    ws = (C.c_uint8 * 64)()
    flags = (C.c_uint32 * 1)()
    rows = (C.c_int64 * 4)()

    def call(keys=key, n_keys=1, nrows=4, sel=None, n_sel=0, mode=0, marks_out=out, work=ws):
        return lib.hs_mark_first(None, keys, n_keys, nrows, sel, n_sel, mode, marks_out, work, flags)

    assert call(n_keys=0) == 1 and b"hs_mark_first: bad arguments" in lib.hs_last_error()
    assert call(marks_out=None) == 1 and b"hs_mark_first" in lib.hs_last_error()
    assert call(mode=3) == 1 and call(mode=-1) == 1
    assert call(keys=None) == 1 and call(work=None) == 1 and call(nrows=-1) == 1
    assert call(sel=rows, n_sel=5) == 1 and call(sel=rows, n_sel=-1) == 1  # more listed rows than rows
    assert call(n_keys=13) == 2 and b"hs_mark_first: more than 12 columns" in lib.hs_last_error()
    key[0].kind = 77
    assert call() == 1 and b"column 0 is not a column that can be compared" in lib.hs_last_error()
    key[0].kind = hs.I32
    assert call(nrows=0) == 0  # nothing to mark, nothing launched
    assert list(out) == [0, 0, 0, 0]
    assert lib.hs_mark_first_ws_bytes(-1, 1, 1) == 0
    assert lib.hs_mark_first_ws_bytes(1 << 20, 2, 3) >= lib.hs_order_by_ws_bytes(1 << 20, 2, 3) + (4 << 24)
