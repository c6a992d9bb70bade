"""tests/sql_model.py and tests/sql_fuzz_gen.py without a GPU: the model against the pinned oracle on the language the oracle
knows, the model against rows written out by hand for everything newer, the generator's own promises over the default seed
window, and ten deliberately wrong models that the seeds must notice."""

from __future__ import annotations

import os
from collections import Counter
from datetime import datetime
from functools import lru_cache

import pytest

from tests import sql_fuzz_gen as G
from tests import sql_model as M
from tests.sql_model import Agg, Bin, Case, Col, DatePart, DateTrunc, Join, Like, Lit, Query, Table, Win

SEEDS = range(int(os.environ.get("HIPSPARK_SQLFUZZ_FIRST", "0")),
              int(os.environ.get("HIPSPARK_SQLFUZZ_FIRST", "0")) + int(os.environ.get("HIPSPARK_SQLFUZZ_SEEDS", "64")))


DEFAULT = range(64)  # the window the coverage conditions are stated for, whatever the environment says
bits = M.row_bits


# ---- 1. the model against the pinned oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(48))
def test_model_equals_the_oracle_on_the_old_language(tmp_path, seed):
    from minispark_amd.parser import parse_sql
    from oracle.py_engine import run_query

    tables, q, sql = G.random_query(seed, tmp_path, old=True)
    assert not q.windows and not q.distinct and not q.order_by and q.limit is None
    assert all(j.kind == "inner" for j in q.joins) and (q.group is None or len(q.group) == 1) and not q.key_items
    model = M.Model()
    want = model.run(q, tables)
    assert not model.inexact
    got = run_query(parse_sql(sql, object()).task)  # the text builds the query through DataFrame(object())
    assert Counter(bits(r) for r in got) == Counter(bits(r) for r in want.rows), sql
    assert [list(r) for r in got[:1]] == [want.names for _ in got[:1]]
    if q.group is None:  # rows: the reference's order - the file's, or the join's shuffle partitions - is the model's
        assert [bits(r) for r in got] == [bits(r) for r in want.rows], sql


@pytest.mark.parametrize("seed", range(6))
def test_model_rounds_where_the_oracle_rounds(tmp_path, seed):
    """The random queries make every sum exact, so they cannot tell one rounding point from another.  Here nothing is exact:
    random f32 cells over three ragged blocks, with and without a join, and every bit of SUM / AVG / MIN / MAX must be the
    oracle's - per-unit partials rounded to f32, merged in f64 in unit order, AVG from the unrounded merged sum."""
    import random

    from minispark_amd.parser import parse_sql
    from oracle.py_engine import run_query

    rng = random.Random(seed)
    rows = [dict(k=rng.randrange(4), x=M.f32(rng.uniform(-1e4, 1e4)), y=M.f32(rng.uniform(0.0, 3.0))) for _ in range(500)]
    others = [dict(rk=rng.randrange(5), z=M.f32(rng.uniform(-2.0, 2.0))) for _ in range(23)]
    tables = {"R": Table("R", [("k", M.INTEGER), ("x", M.FLOAT), ("y", M.FLOAT)], rows, 187, str(tmp_path / "R.bin")),
              "S": Table("S", [("rk", M.INTEGER), ("z", M.FLOAT)], others, 9, str(tmp_path / "S.bin"))}
    for table in tables.values():
        G.write_table(tmp_path / f"{table.name}.bin", table)
    joined = seed % 2 == 1
    arg = Bin("*", Col("x"), Col("z" if joined else "y"))
    q = Query("R", joins=(Join("inner", "S", "k", "rk"),) if joined else (), select=("k", "s", "a", "lo", "hi", "c"), group=("k",),
              aggs=(Agg("sum", Col("x"), "s"), Agg("avg", arg, "a"), Agg("min", Col("x"), "lo"), Agg("max", arg, "hi"),
                    Agg("count", None, "c")))
    sql = (f"SELECT k, SUM(x) AS s, AVG({G.sql_expr(arg)}) AS a, MIN(x) AS lo, MAX({G.sql_expr(arg)}) AS hi, COUNT() AS c "
           f"FROM '{tables['R'].path}'" + (f" JOIN '{tables['S'].path}' ON k = rk" if joined else "") + " GROUP BY k;")
    model = M.Model()
    want = model.run(q, tables)
    assert model.inexact  # the partials were rounded
    got = run_query(parse_sql(sql, object()).task)
    assert Counter(bits(r) for r in got) == Counter(bits(r) for r in want.rows)


# ---- 2. the model against rows written out by hand ------------------------------------------------------------------------------
def ts(text: str) -> datetime:
    return datetime.fromisoformat(text)


T_ROWS = [  # n   k   v    x     s     t
    (0, 1, 10, 0.5, "a", ts("1969-12-28 23:59:59")),  # a Sunday
    (1, 2, 20, -0.0, "b", ts("1970-01-01 00:00:00")),  # a Thursday
    (2, 1, 10, 0.0, "a", ts("2000-02-29 12:00:00")),
    (3, 3, 30, 1.5, "", ts("2024-12-31 23:00:00")),
    (4, 2, 20, 2.0, "b", ts("2001-07-04 06:30:15")),
    (5, 1, 40, -1.0, "ab", ts("2001-07-04 06:30:15")),
    (6, 3, 30, 1.5, "c", ts("1999-12-31 00:00:00")),
    (7, 2, 50, 0.25, "b", ts("2010-10-10 10:10:10")),
    (8, 1, 10, 0.5, "a", ts("1985-05-05 05:05:05")),
    (9, 3, 60, -2.5, "c", ts("1970-01-01 00:00:01")),
    (10, 2, 20, 2.0, "b", ts("2031-01-01 00:00:00")),
    (11, 1, 70, 3.0, "z", ts("1969-01-01 00:00:00")),
]
T_SCHEMA = [("n", M.INTEGER), ("k", M.INTEGER), ("v", M.INTEGER), ("x", M.FLOAT), ("s", M.STRING), ("t", M.TIMESTAMP)]
U_ROWS = [(1, 5), (2, -1), (3, 7), (3, -2)]


def hand_tables() -> dict:
    t = Table("T", T_SCHEMA, [dict(zip([n for n, _ in T_SCHEMA], r)) for r in T_ROWS], rows_per_block=5)
    u = Table("U", [("uk", M.INTEGER), ("uv", M.INTEGER)], [dict(uk=a, uv=b) for a, b in U_ROWS], rows_per_block=3)
    return {"T": t, "U": u}


def column(result: M.Result, name: str) -> list:
    return [r[name] for r in result.rows]


K1 = Bin("=", Col("k"), Lit(1))  # rows n = 0 2 5 8 11: v = 10 10 40 10 70, x = .5 0. -1. .5 3., s = a a ab a z
BY_V = (("v", True),)
WINDOW_CASES = [  # over SELECT n, v, x, s WHERE k = 1; sorted by v: n = 0 2 8 (peers) 5 11
    (Win("row_number", "w", order=BY_V), [1, 2, 4, 3, 5]),
    (Win("row_number", "w", order=(("v", False),)), [3, 4, 2, 5, 1]),  # DESC: 11 5 0 2 8, ties still in input order
    (Win("row_number", "w"), [1, 2, 3, 4, 5]),
    (Win("rank", "w", order=BY_V), [1, 1, 4, 1, 5]),
    (Win("dense_rank", "w", order=BY_V), [1, 1, 2, 1, 3]),
    (Win("ntile", "w", order=BY_V, buckets=2), [1, 1, 2, 1, 2]),  # 5 rows in 2 buckets: 3 + 2
    (Win("ntile", "w", order=BY_V, buckets=7), [1, 2, 4, 3, 5]),  # more buckets than rows
    (Win("lag", "w", "x", order=BY_V, offset=1, default=-9), [-9.0, 0.5, 0.5, 0.0, -1.0]),
    (Win("lead", "w", "v", order=BY_V, offset=2, default=0), [10, 40, 0, 70, 0]),
    (Win("lag", "w", "v", partition=("s",), order=BY_V, offset=0, default=7), [10, 10, 40, 10, 70]),
    (Win("first_value", "w", "x", order=BY_V, frame="range"), [0.5, 0.5, 0.5, 0.5, 0.5]),
    (Win("last_value", "w", "x", order=BY_V, frame="range"), [0.5, 0.5, -1.0, 0.5, 3.0]),  # through the last peer
    (Win("last_value", "w", "x", order=BY_V, frame="rows"), [0.5, 0.0, -1.0, 0.5, 3.0]),
    (Win("last_value", "w", "n", order=BY_V, frame="partition"), [11, 11, 11, 11, 11]),
    (Win("sum", "w", "x", order=BY_V, frame="range"), [1.0, 1.0, 0.0, 1.0, 3.0]),
    (Win("sum", "w", "x", order=BY_V, frame="rows"), [0.5, 0.5, 0.0, 1.0, 3.0]),
    (Win("sum", "w", "v", order=BY_V, frame=("between", 1, 1)), [20, 30, 120, 60, 110]),
    (Win("sum", "w", "v", order=BY_V, frame=("between", 7, 0)), [10, 20, 70, 30, 140]),  # wider than the partition
    (Win("count", "w", order=BY_V, frame=("between", 0, 2)), [3, 3, 2, 3, 1]),
    (Win("first_value", "w", "n", order=BY_V, frame=("between", 1, 7)), [0, 0, 8, 2, 5]),
    (Win("avg", "w", "v", partition=("s",), frame="partition"), [10.0, 10.0, 40.0, 10.0, 70.0]),
    (Win("avg", "w", "v", order=BY_V, frame="rows"), [10.0, 10.0, M.f32(70 / 4), 10.0, 28.0]),
    (Win("max", "w", "x", partition=("s",), frame="partition"), [0.5, 0.5, -1.0, 0.5, 3.0]),
    (Win("min", "w", "x", order=BY_V, frame="range"), [0.0, 0.0, -1.0, 0.0, -1.0]),
    (Win("count", "w", frame="partition"), [5, 5, 5, 5, 5]),
]


@pytest.mark.parametrize("case", range(len(WINDOW_CASES)))
def test_window_items_with_ties(case):
    win, want = WINDOW_CASES[case]
    select = tuple((c, Col(c)) for c in ("n", "v", "x", "s"))
    got = M.run(Query("T", where=K1, select=select, windows=(win,)), hand_tables())
    assert column(got, "n") == [0, 2, 5, 8, 11]
    assert [bits({"w": v}) for v in column(got, "w")] == [bits({"w": v}) for v in want]
    assert got.determined  # ties after a scan follow the file


def test_qualify_distinct_order_and_limit_follow_the_windows():
    select = tuple((c, Col(c)) for c in ("k", "v"))
    q = Query("T", select=select, windows=(Win("row_number", "rn", partition=("k",), order=(("v", False),)),),
              qualify=Bin("<=", Col("rn"), Lit(2)), order_by=(("k", True), ("rn", True)))
    assert M.run(q, hand_tables()).rows == [dict(k=1, v=70, rn=1), dict(k=1, v=40, rn=2), dict(k=2, v=50, rn=1),
                                            dict(k=2, v=20, rn=2), dict(k=3, v=60, rn=1), dict(k=3, v=30, rn=2)]


def test_distinct_keeps_the_first_row_with_its_bits():
    q = Query("T", where=Bin("<=", Col("v"), Lit(20)), select=(("x", Col("x")),), distinct=True)
    assert [r["x"].hex() for r in M.run(q, hand_tables()).rows] == [(0.5).hex(), (-0.0).hex(), (2.0).hex()]  # n = 0 1 (2) 4 (8 10)
    q = Query("T", select=(("k", Col("k")), ("s", Col("s"))), distinct=True, order_by=(("s", False),), limit=4)
    assert M.run(q, hand_tables()).rows == [dict(k=1, s="z"), dict(k=3, s="c"), dict(k=2, s="b"), dict(k=1, s="ab")]


def test_order_by_is_stable_and_limit_reports_a_cut_through_ties():
    q = Query("T", select=(("n", Col("n")), ("k", Col("k")), ("s", Col("s"))), order_by=(("k", False), ("s", True)))
    assert column(M.run(q, hand_tables()), "n") == [3, 6, 9, 1, 4, 7, 10, 0, 2, 8, 5, 11]  # '' < 'c'; 'a' < 'ab' < 'z'
    cut5 = M.run(Query("T", select=q.select, order_by=q.order_by, limit=5), hand_tables())
    assert column(cut5, "n") == [3, 6, 9, 1, 4] and not cut5.determined  # n = 4 and n = 7 tie on (2, 'b')
    cut3 = M.run(Query("T", select=q.select, order_by=q.order_by, limit=3), hand_tables())
    assert column(cut3, "n") == [3, 6, 9] and cut3.determined
    assert M.run(Query("T", select=q.select, order_by=q.order_by, limit=0), hand_tables()).rows == []
    assert len(M.run(Query("T", select=q.select, limit=100), hand_tables()).rows) == 12


def test_semi_and_anti_joins_with_an_anded_condition():
    cond = Bin(">", Col("uv"), Lit(0))  # U's keys with uv > 0: 1 and 3
    select = (("n", Col("n")),)
    anti = M.run(Query("T", joins=(Join("anti", "U", "k", "uk", cond),), select=select), hand_tables())
    semi = M.run(Query("T", joins=(Join("semi", "U", "k", "uk", cond),), select=select), hand_tables())
    assert column(anti, "n") == [1, 4, 7, 10] and column(semi, "n") == [0, 2, 3, 5, 6, 8, 9, 11]
    assert column(M.run(Query("T", joins=(Join("anti", "U", "k", "uk"),), select=select), hand_tables()), "n") == []


def test_the_inner_join_emits_right_row_then_left_row():
    q = Query("U", joins=(Join("inner", "T", "uk", "k"),), where=Bin("<", Col("n"), Lit(4)),
              select=(("uv", Col("uv")), ("n", Col("n"))))
    # T's rows n = 0 1 2 3 have k = 1 2 1 3; U's rows with those keys, in U's order, behind each of them ...
    # ... partition by partition of the shuffle, hash(key) % 10 ascending: the keys 1, 2 and 3 in that order
    assert M.run(q, hand_tables()).rows == [dict(uv=5, n=0), dict(uv=5, n=2), dict(uv=-1, n=1), dict(uv=7, n=3), dict(uv=-2, n=3)]
    keys = Query("U", joins=(Join("inner", "T", "uk", "k"),), where=Bin(">", Col("n"), Lit(9)), select=(("n", Col("n")),))
    assert column(M.run(keys, hand_tables()), "n") == [11, 10]  # k = 1 before k = 2, whatever the right rows' order


def test_group_by_several_columns_with_having():
    q = Query("T", select=("k", "s", "sv", "ax", "c"), group=("k", "s"),
              aggs=(Agg("sum", Col("v"), "sv"), Agg("avg", Col("x"), "ax"), Agg("count", None, "c")),
              having=Bin(">=", Col("c"), Lit(2)))
    got = M.run(q, hand_tables())
    want = [dict(k=1, s="a", sv=30, ax=M.f32(1 / 3), c=3), dict(k=2, s="b", sv=110, ax=1.0625, c=4), dict(k=3, s="c", sv=90, ax=-0.5, c=2)]
    assert sorted(got.rows, key=lambda r: r["k"]) == want and got.types == [M.INTEGER, M.STRING, M.INTEGER, M.FLOAT, M.INTEGER]


def test_aggregates_without_group_by_and_count_distinct_of_the_two_zeros():
    small = Bin("<=", Col("v"), Lit(20))  # n = 0 1 2 4 8 10: x = 0.5 -0.0 0.0 2.0 0.5 2.0
    q = Query("T", where=small, select=("d", "c", "lo", "dt"), group=(),
              aggs=(Agg("count_distinct", Col("x"), "d"), Agg("count", None, "c"), Agg("min", Col("v"), "lo"),
                    Agg("count_distinct", DatePart("year", Col("t")), "dt")))
    assert M.run(q, hand_tables()).rows == [dict(d=3, c=6, lo=10, dt=6)]
    nothing = Query("T", where=Bin(">", Col("v"), Lit(1000)), select=("c",), group=(), aggs=(Agg("count", None, "c"),))
    assert M.run(nothing, hand_tables()).rows == []  # no row survives: no row, not a zero


def test_date_parts_and_date_trunc_before_1970():
    parts = ("year", "month", "day", "hour", "dayofweek", "dayofyear", "quarter")
    select = tuple((p, DatePart(p, Col("t"))) for p in parts) + (("wk", DateTrunc("week", Col("t"))), ("q", DateTrunc("quarter", Col("t"))))
    rows = M.run(Query("T", where=Bin("<=", Col("n"), Lit(2)), select=select), hand_tables()).rows
    assert rows[0] == dict(year=1969, month=12, day=28, hour=23, dayofweek=7, dayofyear=362, quarter=4,
                           wk=ts("1969-12-22"), q=ts("1969-10-01"))  # the Sunday belongs to the week of Monday the 22nd
    assert rows[1] == dict(year=1970, month=1, day=1, hour=0, dayofweek=4, dayofyear=1, quarter=1, wk=ts("1969-12-29"), q=ts("1970-01-01"))
    assert rows[2] == dict(year=2000, month=2, day=29, hour=12, dayofweek=2, dayofyear=60, quarter=1, wk=ts("2000-02-28"), q=ts("2000-01-01"))


def test_case_arithmetic_like_and_timestamp_literals():
    select = (("c", Case(Bin(">", Col("x"), Lit(0)), Col("v"), Bin("/", Col("k"), Lit(2)))),  # FLOAT: one branch is
              ("fd", Bin("//", Bin("-", Col("v"), Lit(45)), Lit(8))), ("md", Bin("%", Bin("-", Col("v"), Lit(45)), Lit(8))),
              ("cat", Bin("+", Bin("+", Col("s"), Lit("-")), Col("s"))))
    where = Bin("and", Bin(">=", Col("t"), Lit("1969-12-28")), Bin("<=", Col("t"), Lit("1970-01-01 00:00:00")))
    rows = M.run(Query("T", where=where, select=select), hand_tables()).rows
    assert rows == [dict(c=10.0, fd=-5, md=5, cat="a-a"), dict(c=1.0, fd=-4, md=7, cat="b-b")]
    like = Query("T", where=Like(Col("s"), "a%"), select=(("n", Col("n")),))
    assert column(M.run(like, hand_tables()), "n") == [0, 2, 5, 8]
    assert [M.like_match(s, p) for s, p in (("", ""), ("", "%"), ("", "_"), ("ab", "_b"), ("ab", "%a"), ("a%b", "a%b"), ("abc", "a%c%"))] \
        == [True, True, False, True, False, True, True]


def test_a_tie_sensitive_window_over_grouped_rows_is_reported():
    aggs = (Agg("count", None, "c"),)
    tied = Query("T", select=("k", "c"), group=("k",), aggs=aggs, windows=(Win("row_number", "rn"),))
    keyed = Query("T", select=("k", "c"), group=("k",), aggs=aggs, windows=(Win("row_number", "rn", order=(("k", True),)),))
    ranked = Query("T", select=("s", "c"), group=("s",), aggs=aggs, windows=(Win("rank", "rk", order=(("c", True),)),))
    assert not M.run(tied, hand_tables()).determined and M.run(keyed, hand_tables()).determined
    assert M.run(ranked, hand_tables()).determined  # ties, but RANK does not look inside them
    assert sorted((r["s"], r["rk"]) for r in M.run(ranked, hand_tables()).rows) == [("", 1), ("a", 5), ("ab", 1), ("b", 6), ("c", 4), ("z", 1)]


def test_the_rounding_points_are_reported():
    model = M.Model()
    rows = [dict(g=0, x=16777216.0), dict(g=0, x=1.0)]
    t = Table("R", [("g", M.INTEGER), ("x", M.FLOAT)], rows, rows_per_block=2)
    got = model.run(Query("R", select=("s",), group=(), aggs=(Agg("sum", Col("x"), "s"),)), {"R": t})
    assert got.rows == [dict(s=16777216.0)] and model.inexact  # 2^24 + 1 is no f32: the partial is rounded, and listed
    with pytest.raises(OverflowError):
        M.run(Query("T", select=(("big", Bin("*", Bin("*", Col("v"), Lit(1 << 20)), Lit(1 << 10))),)), hand_tables())


def test_the_parser_reads_distinct_as_a_name_in_front_of_a_parenthesis_or_a_minus(tmp_path):
    """The two spellings of COUNT(DISTINCT e) the generator never writes (sql_fuzz_gen.REFUSALS)."""
    from minispark_amd.parser import SemanticError, parse_sql

    tables, _, _ = G.random_query(1, tmp_path)
    path = tables["A"].path
    with pytest.raises(SemanticError, match="^Unsupported function: DISTINCT$"):
        parse_sql(f"SELECT COUNT(DISTINCT (i + d)) AS a FROM '{path}';", object())
    with pytest.raises(AssertionError, match="^COUNT takes no argument$"):
        parse_sql(f"SELECT COUNT(DISTINCT -2 * i) AS a FROM '{path}';", object())
    assert parse_sql(f"SELECT COUNT(DISTINCT i + d) AS a, COUNT(DISTINCT 2 * i) AS b FROM '{path}';", object()).schema


# ---- 3. what the generator promises, over the default seed window -------------------------------------------------------------
@lru_cache(maxsize=None)
def generated(seed: int):
    tables, q, sql = G.random_query(seed)
    model = M.Model()
    return tables, q, sql, model.run(q, tables), tuple(model.inexact)


@pytest.mark.parametrize("seed", [*SEEDS, *G.BIG_SEEDS])
def test_every_text_parses_and_plans_and_every_query_is_determined_and_exact(tmp_path, seed):
    from minispark_amd.parser import parse_sql
    from minispark_amd.plan import PhysicalPlan

    if seed in G.BIG_SEEDS:
        tables, q, sql = G.random_query(seed, tmp_path)
        model = M.Model()
        result, inexact = model.run(q, tables), model.inexact
        assert len(tables["A"].rows) == 40_000 and len(tables["B"].rows) == 300
    else:
        tables, q, _, result, inexact = generated(seed)
        _, q2, sql = G.random_query(seed, tmp_path)  # the same query, with files behind the paths
        assert q2 == q
    frame = parse_sql(sql, object())
    assert [name for name, _ in frame.schema] == result.names, sql
    assert [getattr(kind, "name", kind) for _, kind in frame.schema] == result.types, sql
    assert PhysicalPlan.generate_physical_plan(frame.task).stages, sql
    assert result.determined, (result.why, sql)
    assert not inexact, (inexact[:3], sql)
    assert result.join_rows <= 200_000, sql
    assert len(result.names) <= 12 and len(q.order_by) <= 3 and len(q.windows) <= 3


def test_the_default_window_reaches_every_feature_and_every_pair():
    results = [generated(seed) for seed in DEFAULT]
    n = len(results)
    assert sum(not r[3].rows for r in results) <= n // 4, "more than 25 % of the queries have an empty result"
    assert sum(len(r[3].rows) == 1 for r in results) <= n // 10, "more than 10 % of the queries have a one-row result"
    seen = Counter()
    pairs = set()
    for tables, q, sql, result, _ in results:
        has = G.features(q, sql, tables) | result.notes
        seen.update(has)
        pairs |= {frozenset((a, b)) for a in G.PAIRED for b in G.PAIRED if a < b and a in has and b in has}
    assert not [(f, seen[f]) for f in G.FEATURES if seen[f] < 4]
    wanted = {frozenset((a, b)) for a in G.PAIRED for b in G.PAIRED if a < b} - G.EXCLUSIVE
    assert not sorted(tuple(sorted(p)) for p in wanted - pairs)


def test_the_tables_are_what_the_generator_documents():
    sizes = Counter()
    for seed in [*DEFAULT, G.BIG_SEEDS[0]]:
        tables = generated(seed)[0] if seed in DEFAULT else G.make_tables(seed, None)
        a = tables["A"]
        sizes[len(a.rows)] += 1
        assert sorted(r["id"] for r in a.rows) == list(range(len(a.rows)))
        if len(a.rows) >= 4:
            assert {M.I32_MIN, M.I32_MAX, 0, -1} <= {r["sk"] for r in a.rows}
        assert all(r["d"] != 0 and r["g"] != 0 and r["f"] * 8 == int(r["f"] * 8) and len(r["w"]) == 3 for r in a.rows)
        assert all(len(r["s"].encode()) <= 20 and 1969 <= r["t"].year <= 2031 for r in a.rows)
        if len(a.rows) >= 200:
            assert len({r["s"] for r in a.rows}) >= 100 and len({r["w"] for r in a.rows}) == 5
    assert set(sizes) == {1, 7, 200, 3000, 40_000}
    for section, refused, avoided in G.REFUSALS:
        assert section and refused and avoided


# ---- 4. the seeds bite ---------------------------------------------------------------------------------------------------------
MISTAKES = ("frame_end_off_by_one", "rank_as_dense_rank", "anti_as_semi", "limit_before_distinct", "qualify_before_other_spec",
            "having_ignored", "count_distinct_as_count", "weeks_start_on_sunday", "lag_default_ignored", "desc_as_asc")


@pytest.mark.parametrize("mistake", MISTAKES)
def test_a_wrong_model_is_noticed_by_at_least_three_seeds(mistake):
    noticed = []
    for seed in DEFAULT:
        tables, q, _, right, _ = generated(seed)
        wrong = M.run(q, tables, **{mistake: True})
        differs = M.difference(q, right.rows, wrong.rows) is not None
        if differs:
            noticed.append(seed)
    assert len(noticed) >= 3, f"{mistake}: only seeds {noticed} tell the wrong model from the right one"
