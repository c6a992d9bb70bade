"""CASE WHEN without a GPU: the grammar against the API, the typing rule, the exact programs the lowering emits
(HS_OP_SEL), the CPU model the GPU tests compare against - and two guards that hold before the feature too: texts and
expressions without CASE keep the trees and the program bytes they had (tests/golden/case_when_parent.json, recorded
from the commit before CASE existed)."""

from __future__ import annotations

import json
import struct
from datetime import datetime
from pathlib import Path

import pytest

import oracle.py_engine as py_engine
from minispark_amd import hipspark as hs
from minispark_amd import tasks as t
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.lowering import LoweringError, ProgramBuilder, expr_key, lower_aggregate
from minispark_amd.parser import SqlSyntaxError, parse_sql
from minispark_amd.sql import CaseColumn, Col, Functions as F, Lit
from tests import case_when_model
from tests.sql_texts import E2E_SQL
from tests.test_parser import render

PARENT = json.loads((Path(__file__).parent / "golden" / "case_when_parent.json").read_text())
_MIRROR = {"lt": "gt", "le": "ge", "gt": "lt", "ge": "le", "eq": "eq", "ne": "ne"}


def canon(col) -> str:
    """tests/test_parser.canon (``literal <op> column`` turned around) that also walks into a CASE."""
    kind = type(col).__name__
    if kind == "BinaryOperatorColumn":
        left, right, op = col.left_side, col.right_side, col.operator.__name__
        if op in _MIRROR and type(left).__name__ == "Lit" and type(right).__name__ != "Lit":
            left, right, op = right, left, _MIRROR[op]
        return f"({canon(left)} {op} {canon(right)})"
    if kind == "AliasColumn":
        return f"{canon(col.original_col)} AS {col.name}"
    if kind == "LikeColumn":
        return f"{canon(col.original_col)} LIKE {col.pattern!r}"
    if kind == "AggCol":
        return f"{col.type}({canon(col.original_col)})"
    if kind == "CaseColumn":
        return f"CASE({canon(col.condition)} ? {canon(col.then_col)} : {canon(col.else_col)})"
    return str(col)


def tree(task) -> list[str]:
    out, node = [], task
    while node is not None and type(node).__name__ != "VoidTask":
        name = type(node).__name__
        if name == "FilterTask":
            out.append(f"Filter({canon(node.condition)})")
        elif name == "ProjectTask":
            out.append("Project(" + ", ".join(canon(c) for c in node.columns) + ")")
        elif name == "AggregateTask":
            out.append(f"Aggregate({node.group_by_column}; " + ", ".join(canon(c) for c in node.agg_columns) + ")")
        else:
            out.append(node.describe())
        node = node.parent_task
    return out


def T(name="t"):
    return DataFrame(object()).table(name)


def when(cond, value):
    return F.when(cond, value)


# ---- parser ----------------------------------------------------------------------------------------------------------
TEXTS = [
    ("SELECT CASE WHEN a > 1 THEN b ELSE c END AS x FROM 't';",
     lambda: T().select(when(Col("a") > 1, Col("b")).otherwise(Col("c")).alias("x"))),
    ("SELECT CASE WHEN a > 1 THEN 10 WHEN a > 0 THEN 5 WHEN s LIKE 'x%' THEN b ELSE 0 END AS x FROM 't';",
     lambda: T().select(when(Col("a") > 1, 10).when(Col("a") > 0, 5).when(Col("s").like("x%"), Col("b")).otherwise(0).alias("x"))),
    ("SELECT 1 + CASE WHEN a = b THEN a * 2 ELSE b - 1 END AS x, (CASE WHEN a != 0 THEN 1 ELSE 0 END) * f AS y FROM 't';",
     lambda: T().select((Lit(1) + when(Col("a") == Col("b"), Col("a") * 2).otherwise(Col("b") - 1)).alias("x"),
                        (when(Col("a") != 0, 1).otherwise(0) * Col("f")).alias("y"))),
    ("SELECT k, SUM(CASE WHEN s = '1-URGENT' THEN 1 ELSE 0 END) AS hi, AVG(CASE WHEN a > 1 THEN f ELSE 0 END) AS m, "
     "MIN(CASE WHEN a > 1 THEN f ELSE g END) AS lo, MAX(1 + CASE WHEN a > 1 THEN a ELSE 0 END) AS top FROM 't' GROUP BY k;",
     lambda: T().group_by(Col("k")).agg(
         F.sum(when(Col("s") == "1-URGENT", 1).otherwise(0)).alias("hi"), F.avg(when(Col("a") > 1, Col("f")).otherwise(0)).alias("m"),
         F.min(when(Col("a") > 1, Col("f")).otherwise(Col("g"))).alias("lo"),
         F.max(Lit(1) + when(Col("a") > 1, Col("a")).otherwise(0)).alias("top"))
     .select(Col("k"), Col("hi"), Col("m"), Col("lo"), Col("top"))),
    ("SELECT SUM(CASE WHEN a BETWEEN lo AND hi THEN 1 ELSE 0 END) AS n FROM 't';",
     lambda: T().agg(F.sum(when(Col("a").between(Col("lo"), Col("hi")), 1).otherwise(0)).alias("n"))),
    ("SELECT a FROM 't' WHERE CASE WHEN a > 1 OR b < 2 AND c = 3 THEN a ELSE b END > 5;",
     lambda: T().filter(when((Col("a") > 1) | ((Col("b") < 2) & (Col("c") == 3)), Col("a")).otherwise(Col("b")) > 5).select(Col("a"))),
    ("SELECT CASE WHEN a > 1 THEN CASE WHEN b > 1 THEN 1 ELSE 2 END ELSE CASE WHEN c > 1 THEN 3 ELSE 4 END END AS x FROM 't';",
     lambda: T().select(when(Col("a") > 1, when(Col("b") > 1, 1).otherwise(2)).otherwise(when(Col("c") > 1, 3).otherwise(4)).alias("x"))),
    ("SELECT  CASE\n WHEN  a > 1\tTHEN b  ELSE   c   END  AS x FROM 't';",
     lambda: T().select(when(Col("a") > 1, Col("b")).otherwise(Col("c")).alias("x"))),
]


@pytest.mark.parametrize("sql,build", TEXTS, ids=[c[0][7:50] for c in TEXTS])
def test_text_builds_the_same_tree_as_the_api(sql, build):
    got, want = parse_sql(sql, object()).task, build().task
    assert tree(got) == tree(want)
    assert any("CASE(" in line for line in tree(got))


def test_several_when_arms_nest_to_the_right():
    col = parse_sql("SELECT CASE WHEN a > 1 THEN 10 WHEN a > 0 THEN 5 ELSE 0 END AS x FROM 't';", object()).task.columns[0]
    case = col.original_col
    assert type(case) is CaseColumn and type(case.else_col) is CaseColumn and type(case.else_col.else_col) is Lit
    assert (case.then_col.value, case.else_col.then_col.value, case.else_col.else_col.value) == (10, 5, 0)
    assert str(case) == "CASE WHEN (1) < (a) THEN 10 WHEN (0) < (a) THEN 5 ELSE 0 END"
    assert [c.name for c in case.all_nested_columns if type(c) is Col] == ["a", "a"]
    same = F.when(Lit(1) < Col("a"), 10).when(Lit(0) < Col("a"), 5).otherwise(0)
    assert hash(same) == hash(case) and expr_key(same) == expr_key(case) and expr_key(case)[0] == "case"
    assert hash(F.when(Lit(1) < Col("a"), 10).otherwise(0)) != hash(case)


@pytest.mark.parametrize("text", [
    "SELECT CASE WHEN a > 1 THEN 2 END FROM 't';",            # no ELSE
    "SELECT CASE WHEN a > 1 THEN 2 ELSE 3 FROM 't';",         # no END
    "SELECT CASE WHEN a > 1 THEN 2 ELSE 3 END END FROM 't';",
    "SELECT CASE a WHEN 1 THEN 2 ELSE 3 END FROM 't';",       # the simple form is not part of the language
    "SELECT CASE WHEN a > 1 2 ELSE 3 END FROM 't';",
    "SELECT CASE WHEN a THEN 2 ELSE 3 END FROM 't';",         # a condition is a comparison, as in WHERE
    "SELECT CASEWHEN a > 1 THEN 2 ELSE 3 END FROM 't';",
    "SELECT SUM(CASE WHEN a > 1 THEN 2 ELSE 3) FROM 't';",
    "SELECT CASE WHEN a > 1 THEN 2 ELSE 3 ENDFROM 't';",       # every keyword ends at a word boundary
    "SELECT CASE WHEN a > 1 THEN 2 ELSE 3 ENDx FROM 't';",
    "SELECT CASE WHEN a > 1 THENb ELSE 3 END FROM 't';",
    "SELECT CASE WHEN a > 1 THEN 2 ELSEb END FROM 't';",
])
def test_malformed_case_is_a_syntax_error(text):
    with pytest.raises(SqlSyntaxError):
        parse_sql(text, object())


def test_a_column_called_case_parses_as_before():
    assert render(parse_sql("SELECT CASE FROM 't';", object()).task) == ["Project(CASE)", "LoadTableBlockTask(t) alias="]
    assert render(parse_sql("SELECT CASE + 1 AS x, WHEN, END FROM 't' WHERE CASE > 2;", object()).task) == [
        "Project((CASE add 1) AS x, WHEN, END)", "Filter((CASE gt 2))", "LoadTableBlockTask(t) alias="]


@pytest.mark.parametrize("name", sorted(E2E_SQL))
def test_existing_texts_render_the_trees_of_the_parent(name):
    task = parse_sql(E2E_SQL[name].format(users="users.bin", orders="orders.bin"), object()).task
    assert render(task) == PARENT["renderings"][name]


def test_every_existing_text_is_covered_by_the_recording():
    assert sorted(PARENT["renderings"]) == sorted(E2E_SQL)


# ---- API -----------------------------------------------------------------------------------------------------------------
def test_the_unfinished_builder_is_not_a_column():
    builder = F.when(Col("a") > 1, 2)
    assert not isinstance(builder, Col) and not isinstance(builder.when(Col("a") > 0, 1), Col)
    assert type(builder.otherwise(3)) is CaseColumn
    for use in (lambda: F.sum(builder), lambda: builder + 1, lambda: builder > 1, lambda: builder.alias("x"),
                lambda: str(T().select(builder).task.describe()) + builder.name, lambda: hash(builder), lambda: builder.name):
        with pytest.raises(TypeError):
            use()


def test_the_unfinished_builder_answers_attribute_probes_as_any_object_does():
    builder = F.when(Col("a") > 1, 2)
    assert not hasattr(builder, "no_such_thing") and getattr(builder, "_pytestfixturefunction", None) is None
    assert hasattr(builder, "when") and hasattr(builder, "otherwise")
    for name in ("alias", "name", "children", "infer_type", "like", "between", "normalize_agg_columns", "all_nested_columns"):
        with pytest.raises(TypeError, match="otherwise"):
            getattr(builder, name)


def test_normalize_agg_columns_walks_into_a_case():
    cond = F.sum(Col("a")) > Lit(3)
    case = F.when(cond, F.sum(Col("a"))).otherwise(F.max(Col("b")))
    assert str(case.normalize_agg_columns()) == "CASE WHEN (sum_a) > (3) THEN sum_a ELSE max_b END"


# ---- infer_type ----------------------------------------------------------------------------------------------------------
SCHEMA = [(n, getattr(ColumnType, ty)) for n, ty in PARENT["schema"]]  # a b INTEGER, f FLOAT, s d STRING, ts TIMESTAMP
KINDS = list(PARENT["kinds"])
DICTS = [None if d is None else tuple(e.encode() for e in d) for d in PARENT["dicts"]]
C = Col("a") > Col("b")


@pytest.mark.parametrize("then,other,want", [
    (Col("a"), Col("b"), ColumnType.INTEGER), (Col("a"), Col("f"), ColumnType.FLOAT), (Col("f"), Lit(0), ColumnType.FLOAT),
    (Col("f"), Col("f") * 2.0, ColumnType.FLOAT), (Col("a") / Col("b"), Lit(1), ColumnType.FLOAT),
    (Lit(1), Lit(0), ColumnType.INTEGER), (F.when(C, 1).otherwise(2), Col("f"), ColumnType.FLOAT),
])
def test_the_value_is_float_if_either_branch_is(then, other, want):
    assert F.when(C, then).otherwise(other).infer_type(SCHEMA) == want


@pytest.mark.parametrize("then,other,word", [
    (Col("s"), Lit(0), "STRING"), (Lit(1), Lit("x"), "STRING"), (Col("ts"), Col("ts"), "TIMESTAMP"),
    (Lit(1), Lit(datetime(2025, 1, 1)), "TIMESTAMP"), (Col("a") > Lit(1), Lit(0), "boolean"),
    (Lit(1), Col("s").like("a%"), "boolean"), (Lit(1), (Col("a") > 1) & (Col("b") > 1), "boolean"), (Lit(True), Lit(0), "boolean"),
])
def test_string_timestamp_and_boolean_branches_are_refused(then, other, word):
    case = F.when(C, then).otherwise(other)
    with pytest.raises(TypeError, match=word) as err:
        case.infer_type(SCHEMA)
    assert "CASE WHEN" in str(err.value)  # names the node
    with pytest.raises((TypeError, LoweringError)):
        ProgramBuilder(SCHEMA, KINDS, DICTS).lower(case)


def test_lowering_refuses_and_or_over_integers_as_a_branch_as_infer_type_does():
    """`a & b` over INTEGER operands lowers to an I cell, but AND / OR is boolean by its shape: both passes refuse it."""
    case = F.when(C, Col("a") & Col("b")).otherwise(0)
    with pytest.raises(TypeError, match="boolean"):
        case.infer_type(SCHEMA)
    with pytest.raises(TypeError, match="boolean"):
        ProgramBuilder(SCHEMA, KINDS, DICTS).lower(case)


def test_the_predicted_branch_tag_is_checked_against_the_lowered_one(monkeypatch):
    """value_tag restates lower()'s typing; if the two ever disagree the lowering stops instead of choosing an INTEGER cell as FLOAT."""
    real = ProgramBuilder.value_tag
    monkeypatch.setattr(ProgramBuilder, "value_tag", lambda self, node: "F" if type(node) is Col and node.name == "a" else real(self, node))
    with pytest.raises(AssertionError, match="value_tag"):
        ProgramBuilder(SCHEMA, KINDS, DICTS).lower(F.when(C, Col("a")).otherwise(Col("f")))


def test_the_condition_is_type_checked_like_a_where():
    with pytest.raises(TypeError, match="Type mismatch"):
        F.when(Col("a") > Col("s"), 1).otherwise(0).infer_type(SCHEMA)
    with pytest.raises(ValueError, match="not found"):
        F.when(Col("nope") > 1, 1).otherwise(0).infer_type(SCHEMA)


def test_a_case_is_no_filter_and_no_group_key():
    with pytest.raises(AssertionError):
        T().filter(F.when(C, 1).otherwise(0))
    with pytest.raises(ValueError, match="GroupBy"):
        lower_aggregate(SCHEMA, KINDS, [], F.when(C, Col("a")).otherwise(Col("b")), [F.sum(Col("a"))], DICTS)


# ---- lowering ------------------------------------------------------------------------------------------------------------
def ins(program) -> list[tuple]:
    return [(w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xffff, (w >> 32) & 0xffff, (w >> 48) & 0xffff) for w in program.ins]


def lower_out(expr):
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    tag = b.emit_out(0, expr)
    return tag, b.finish()


def test_integer_branches():
    tag, p = lower_out(F.when(C, Col("a")).otherwise(Col("b")))
    assert tag == "I" and p.columns == [0, 1] and p.max_depth == 3 and p.lits == []
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_LD, 1, 1, 0, 0), (hs.OP_GT_I, 2, 0, 0, 0),   # c
                      (hs.OP_LD, 1, 0, 0, 0), (hs.OP_LD, 2, 1, 0, 0),                                # x y
                      (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]
    assert hs.OP_SEL == 37


def test_float_and_integer_branches_convert_the_integer_cell_while_it_is_on_top():
    tag, p = lower_out(F.when(C, Col("f")).otherwise(0))
    assert tag == "F" and p.columns == [0, 1, 2] and p.lits == [0]
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_LD, 1, 1, 0, 0), (hs.OP_GT_I, 2, 0, 0, 0),
                      (hs.OP_LD, 1, 2, 0, 0), (hs.OP_LIT, 2, 0, 0, 0), (hs.OP_I2F, 3, 0, 0, 0),
                      (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]
    tag, p = lower_out(F.when(C, Col("a")).otherwise(Col("f")))  # the THEN cell: converted before ELSE is pushed
    assert tag == "F"
    assert ins(p)[3:] == [(hs.OP_LD, 1, 0, 0, 0), (hs.OP_I2F, 2, 0, 0, 0), (hs.OP_LD, 2, 2, 0, 0),
                          (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]


def test_a_float_condition_goes_through_its_truth_value():
    tag, p = lower_out(F.when(Col("f") * Col("f"), 1).otherwise(2))
    assert tag == "I" and p.lits == [0, 1, 2]
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_LD, 1, 0, 0, 0), (hs.OP_MUL_F, 2, 0, 0, 0),
                      (hs.OP_LIT, 1, 0, 0, 0), (hs.OP_NE_F, 2, 0, 0, 0),
                      (hs.OP_LIT, 1, 1, 0, 0), (hs.OP_LIT, 2, 2, 0, 0), (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]


def test_a_nested_case():
    case = F.when(C, 1).when(Col("a") < Col("b"), 2).otherwise(Col("f"))  # the inner CASE is FLOAT, hence the outer
    tag, p = lower_out(case)
    two = struct.unpack("<Q", struct.pack("<q", 2))[0]
    assert tag == "F" and p.lits == [1, two] and p.max_depth == 5
    assert ins(p) == [(hs.OP_LD, 0, 0, 0, 0), (hs.OP_LD, 1, 1, 0, 0), (hs.OP_GT_I, 2, 0, 0, 0),
                      (hs.OP_LIT, 1, 0, 0, 0), (hs.OP_I2F, 2, 0, 0, 0),
                      (hs.OP_LD, 2, 0, 0, 0), (hs.OP_LD, 3, 1, 0, 0), (hs.OP_LT_I, 4, 0, 0, 0),
                      (hs.OP_LIT, 3, 1, 0, 0), (hs.OP_I2F, 4, 0, 0, 0), (hs.OP_LD, 4, 2, 0, 0), (hs.OP_SEL, 5, 0, 0, 0),
                      (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]


def test_a_like_on_a_dictionary_coded_column_is_a_bit_test():
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    tag = b.emit_out(0, F.when(Col("d").like("ap%"), Col("a")).otherwise(0))
    p = b.finish()
    assert tag == "I" and b.code_reads == {4} and b.string_reads == set()
    assert p.columns == [4, 0] and p.code_columns == [4]  # the code byte travels as a preloaded HS_U8 column
    assert p.lits == [0b011, 0]  # apple, apricot match; banana does not
    assert ins(p) == [(hs.OP_DICTBIT, 0, 0, 0, 1), (hs.OP_LD, 1, 1, 0, 0), (hs.OP_LIT, 2, 1, 0, 0),
                      (hs.OP_SEL, 3, 0, 0, 0), (hs.OP_OUT, 1, 0, 0, 0)]
    # the same on a plain string column reads the bytes; a column that occurs only inside the CASE is seen by both
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    b.emit_out(0, F.when(Col("s") == "x", Col("b")).otherwise(0))
    p = b.finish()
    assert b.string_reads == {3} and p.columns == [1, 3] and ins(p)[0] == (hs.OP_STRCMP_LIT, 0, 1, 0, 4)


def test_an_aggregate_argument_and_a_where_comparison():
    low = lower_aggregate(SCHEMA, KINDS, [F.when(C, Col("a")).otherwise(Col("b")) > Lit(5)], Col("b"),
                          [F.sum(F.when(Col("d") == "banana", 1).otherwise(0)), F.sum(F.when(Col("d") == "banana", 1).otherwise(0)),
                           F.max(Lit(1.5) * F.when(C, Col("f")).otherwise(0))], DICTS)
    assert low.acc_ops == [hs.AGG_SUM, hs.AGG_MAX] and low.acc_is_int == [True, False] and low.agg_to_acc == [0, 0, 1]
    ops = [i[0] for i in ins(low.program)]
    assert ops.count(hs.OP_SEL) == 3 and ops.index(hs.OP_FILTER) < ops.index(hs.OP_KEY) < ops.index(hs.OP_AGG)
    assert low.program.code_columns == [4]


def nest(levels: int):
    case = Lit(0)
    for k in range(levels):
        case = F.when(Col("a") > Lit(k), k).otherwise(case)
    return case


def test_a_stack_deeper_than_the_limit_is_refused():
    assert hs.HS_MAX_STACK == 8
    _, p = lower_out(nest(3))
    assert p.max_depth == 7  # two cells per open CASE (condition, THEN value), three for the innermost one
    with pytest.raises(LoweringError, match="stack deeper than 8"):
        lower_out(nest(4))
    arms = F.when(Col("a") > 0, 0)
    for k in range(1, 12):  # WHEN arms nest in the ELSE position like nest(): the same limit
        arms = arms.when(Col("a") > k, k)
    with pytest.raises(LoweringError, match="stack deeper than 8"):
        lower_out(arms.otherwise(0))
    _, p = lower_out(F.when(C, F.when(C, F.when(C, 1).otherwise(2)).otherwise(3)).otherwise(4))  # nesting in THEN: one cell each
    assert p.max_depth == 5


def test_the_iso_string_rewrite_does_not_reach_into_branches():
    with pytest.raises((TypeError, LoweringError)):
        lower_out(F.when(C, Col("a")).otherwise("2025-03-01") > Col("ts"))
    lower_out(F.when(Col("ts") > "2025-03-01", 1).otherwise(0))  # in the condition it applies as in a WHERE


@pytest.mark.parametrize("name", sorted(PARENT["exprs"]))
def test_programs_without_case_keep_the_bytes_of_the_parent(name):
    _, p = lower_out(eval(PARENT["exprs"][name], {"Col": Col, "Lit": Lit}))
    assert p.to_bytes().hex() == PARENT["programs"][name]


def test_the_aggregate_program_without_case_keeps_the_bytes_of_the_parent():
    low = lower_aggregate(SCHEMA, KINDS, [Col("d").like("a%"), Col("f") > Lit(1.0)], Col("a"),
                          [F.sum(Col("f") * Col("b")), F.min(Col("b")), F.max(Col("f")), F.sum(Lit(1))], DICTS)
    want = PARENT["aggregate"]
    assert low.program.to_bytes().hex() == want["program"]
    assert (low.key_slot, low.acc_ops, low.acc_is_int, low.agg_to_acc) == (
        want["key_slot"], want["acc_ops"], want["acc_is_int"], want["agg_to_acc"])


def test_the_stage_lowering_inlines_a_projected_case():
    from minispark_amd.stage import _substitute, _walk_names

    case = F.when(Col("x") > 1, Col("y")).otherwise(0)
    got = _substitute(case, {"x": Col("a") + 1, "y": Col("f")})
    assert type(got) is CaseColumn and str(got) == "CASE WHEN ((a) + (1)) > (1) THEN f ELSE 0 END"
    assert _walk_names(got) == ["a", "f"]


# ---- the model -----------------------------------------------------------------------------------------------------------
MODEL_SCHEMA = [("a", ColumnType.INTEGER), ("b", ColumnType.INTEGER), ("f", ColumnType.FLOAT), ("s", ColumnType.STRING)]
MODEL_ROWS = [(1, 2, 0.5, "x"), (5, 0, -1.25, "yy"), (0, 0, 3.0, "x"), (-3, 7, 0.0, "zx")]


@pytest.mark.parametrize("expr,want", [
    (lambda: F.when(Col("a") > Col("b"), Col("a")).otherwise(Col("b")), [2, 5, 0, 7]),
    (lambda: F.when(Col("a") > Col("b"), Col("f")).otherwise(0), [0.0, -1.25, 0.0, 0.0]),
    (lambda: F.when(Col("s").like("%x"), 1).otherwise(0), [1, 0, 1, 1]),
    (lambda: F.when(Col("a") > 0, 1).when(Col("b") > 0, Col("f")).otherwise(-1), [1.0, 1.0, -1.0, 0.0]),
    (lambda: Lit(1) + F.when(Col("s") == "x", Col("a")).otherwise(Col("b")) * 2, [3, 1, 1, 15]),
    (lambda: F.when(F.when(Col("a") > 0, Col("a")).otherwise(Col("b")) > 4, 1).otherwise(0), [0, 1, 0, 1]),
])
def test_the_model_on_rows_computed_by_hand(monkeypatch, expr, want):
    case_when_model.install(monkeypatch)
    fn = py_engine.compile_expr(expr(), MODEL_SCHEMA)
    got = [fn(row) for row in MODEL_ROWS]
    assert got == want and [type(v) for v in got] == [type(v) for v in want]


def test_the_model_is_eager(monkeypatch):
    case_when_model.install(monkeypatch)
    guarded = F.when(Col("b") != 0, Col("a") / Col("b")).otherwise(0.0)
    fn = py_engine.compile_expr(guarded, MODEL_SCHEMA)
    assert fn(MODEL_ROWS[0]) == 0.5 and type(fn(MODEL_ROWS[0])) is float
    with pytest.raises(ZeroDivisionError):
        fn(MODEL_ROWS[1])  # b = 0: the branch not taken is evaluated too
    assert py_engine.project_column(F.sum(guarded), [[4, 9], [2, 3], [0.0, 0.0], ["", ""]], MODEL_SCHEMA) == [2.0, 3.0]


def test_the_model_leaves_every_other_node_to_the_oracle(monkeypatch):
    plain = (Col("a") + Col("b")) * Col("f")
    before = [py_engine.compile_expr(plain, MODEL_SCHEMA)(row) for row in MODEL_ROWS]
    case_when_model.install(monkeypatch)
    assert [py_engine.compile_expr(plain, MODEL_SCHEMA)(row) for row in MODEL_ROWS] == before
    with pytest.raises(NotImplementedError):
        case_when_model._oracle_compile_expr(F.when(Col("a") > 0, 1).otherwise(0), MODEL_SCHEMA)


def test_group_by_select_rule_is_unchanged():
    from minispark_amd.parser import GroupByError

    with pytest.raises(GroupByError):
        parse_sql("SELECT k, CASE WHEN a > 1 THEN 1 ELSE 0 END AS x FROM 't' GROUP BY k;", object())
    task = parse_sql("SELECT k, SUM(a) AS s FROM 't' GROUP BY k HAVING CASE WHEN SUM(a) > 0 THEN SUM(a) ELSE 0 END > 3;", object()).task
    assert type(task) is t.ProjectTask and "CASE WHEN" in task.parent_task.describe()


# ---- the run-time compiler: translate + compile for gfx950, no GPU needed ---------------------------------------------------
def _hs_cols(program, kinds):
    import ctypes as C

    cols = (hs.hs_col * max(len(program.columns), 1))()
    for slot, idx in enumerate(program.columns):
        coded = idx in program.code_columns
        cols[slot].kind = hs.U8 if coded else kinds[idx]
        cols[slot].fixed_len = 1 if (kinds[idx] == hs.STR and not coded) else -1
    return cols, C


def check_sel_programs_compile():
    """hs_jit_compile_check / _scalar / _eval on programs with HS_OP_SEL: COMPILED, not declined to the interpreter; the
    select is one conditional expression per row, and with three hoisted operands it is hoisted itself."""
    lib = hs.load_library()
    urgent = (Col("d") == "apple") | Col("d").like("b%")
    aggs = [F.sum(F.when(urgent, 1).otherwise(0)), F.sum(F.when(Col("b") > 0, Col("f")).otherwise(0)),
            F.max(F.when(Col("s") == "x", Col("a")).when(Col("a") > 3, Col("b")).otherwise(Col("f"))),
            F.sum(F.when(Lit(0), 5).otherwise(7))]
    where = [F.when(Col("a") > 0, Col("a")).otherwise(Col("b")) > Lit(5)]
    for keyed in (True, False):
        low = lower_aggregate(SCHEMA, KINDS, where, Col("a") if keyed else None, aggs, DICTS)
        cols, C = _hs_cols(low.program, KINDS)
        prog, spec = low.program.to_struct(), low.spec()
        src, size = C.create_string_buffer(1 << 16), C.c_int64(0)
        if keyed:
            rc = lib.hs_jit_compile_check(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                          C.byref(size), src, len(src))
        else:
            rc = lib.hs_jit_compile_check_scalar(cols, len(low.program.columns), C.byref(prog), C.byref(spec), b"gfx950",
                                                 C.byref(size), src, len(src))
        assert rc == 0, (keyed, lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
        text = src.value.decode()
        n_sel = [i[0] for i in ins(low.program)].count(hs.OP_SEL)
        assert n_sel == 6 and text.count(" != 0 ? ") == n_sel and size.value > 4096
        head, _, body = text.partition("for (int j = 0; j < HS_V; ++j)")
        hoisted = [line for line in head.splitlines() if " != 0 ? " in line]
        assert len(hoisted) == 1 and hoisted[0].strip().startswith("const unsigned long long k")  # SUM(CASE WHEN 0 THEN 5 ELSE 7 END)
        assert body.count(" != 0 ? ") == n_sel - 1 and "hs_dictbit" in text
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    tags = [b.emit_out(0, F.when(Col("a") > Col("b"), Col("f")).otherwise(0)),
            b.emit_out(1, Lit(1) + F.when(Col("s").like("x%"), Col("a")).when(urgent, 2).otherwise(Col("b"))),
            b.emit_out(2, F.when(Col("a") > 0, Col("a")).otherwise(Col("b")) > Lit(5))]
    assert tags == ["F", "I", "B"]
    program = b.finish()
    cols, C = _hs_cols(program, KINDS)
    pstruct, size, src = program.to_struct(), C.c_int64(0), C.create_string_buffer(1 << 16)
    out_kinds = (C.c_int32 * 3)(hs.F64, hs.I64, hs.U8)
    rc = lib.hs_jit_compile_check_eval(cols, len(program.columns), C.byref(pstruct), out_kinds, 3, b"gfx950", C.byref(size), src, len(src))
    assert rc == 0, (lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
    assert src.value.decode().count(" != 0 ? ") == 4 and size.value > 1000


def test_programs_with_sel_translate_and_compile_for_gfx950_without_a_gpu():
    check_sel_programs_compile()


def test_the_host_side_program_checks_take_sel_as_a_value_instruction():
    """hs_agg_rows_classify walks `[filter ... FILTER]* KEY [argument ... AGG]*`: a CASE argument is an expression cell
    (kind HS_F64 / HS_I64, no bare column, no literal), a CASE in the WHERE is one filter."""
    import ctypes as C

    lib = hs.load_library()
    low = lower_aggregate(SCHEMA, KINDS, [F.when(Col("a") > 0, Col("a")).otherwise(Col("b")) > Lit(5)], Col("a"),
                          [F.sum(F.when(Col("b") > 0, Col("f")).otherwise(0)), F.sum(F.when(Col("b") > 0, 1).otherwise(0)),
                           F.sum(Col("f")), F.sum(Lit(1))])
    cols, _ = _hs_cols(low.program, KINDS)
    prog, spec = low.program.to_struct(), low.spec()
    kinds, slots, cells, n_filters = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_uint64 * 4)(), C.c_int32(-1)
    rc = lib.hs_agg_rows_classify(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), kinds, slots, cells,
                                  C.byref(n_filters))
    assert rc == 0, lib.hs_last_error()
    assert n_filters.value == 1
    assert list(kinds) == [hs.F64, hs.I64, hs.F32, -1] and list(slots)[:2] == [-1, -1] and cells[3] == 1
