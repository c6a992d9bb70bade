"""Aggregates without GROUP BY on the GPU (hs_agg_scalar) against the oracle's answer for the SAME table with a constant
INTEGER column ``g`` appended and ``GROUP BY g``, the key dropped: same block cuts, so the same units, the same per-unit
f64 / i64 partial sums, the same f32 / i32 quantisation of the unit rows and the same merge in unit order.

Shapes are the smallest at which the kernel can go wrong: units of 1..257 rows (quad preload, the masked first quad of a
unit, partial waves, idle waves), one unit over several chunks (the last-arriver fold), WHERE leaving one row / emptying a
unit / emptying everything, identities that must not escape MIN / MAX, exact and random FLOAT folds, INTEGER overflow,
16 accumulators, both evaluator forms, replay, streamed ranges, a join below, ORDER BY / LIMIT above, SQL, two ranks."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.io import BlockFile, StrCol
from minispark_amd.sql import Col, Functions as F, Lit
from oracle.py_engine import run_query
from tests.conftest import assert_rows_match
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

SCHEMA = [("i", ColumnType.INTEGER), ("f", ColumnType.FLOAT), ("s", ColumnType.STRING), ("j", ColumnType.INTEGER)]
UNIT_SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2]  # 975 rows: not a multiple of 4; most units begin inside a quad
WORDS = ["apple", "apricot", "banana", "cherry", "avocado"]


def make_columns(n: int, seed: int = 7) -> dict:
    rng = np.random.default_rng(seed)
    return {"i": rng.integers(-1000, 1000, n).astype(np.int32),
            "f": (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32),  # k/64, |k| < 2^20: f64 sums are exact
            "s": [WORDS[k] for k in rng.integers(0, len(WORDS), n)],
            "j": np.arange(n, dtype=np.int32)}


def write_pair(folder: Path, name: str, cols: dict, sizes: list[int], schema=SCHEMA) -> tuple[str, str]:
    """The table as it is and the table with a constant INTEGER column g, with the same block cuts."""
    n = sum(sizes)
    assert all(len(cols[c]) == n for c, _ in schema)
    folder.mkdir(parents=True, exist_ok=True)

    def blocks(with_g: bool):
        lo = 0
        for size in sizes:
            part = []
            for c, t in schema:
                v = cols[c][lo: lo + size]
                part.append(StrCol.from_strings(list(v)) if t == ColumnType.STRING else np.asarray(v))
            if with_g:
                part.append(np.full(size, 7, dtype=np.int32))
            lo += size
            yield part

    plain, keyed = folder / f"{name}.bin", folder / f"{name}_g.bin"
    BlockFile(plain).write_raw_blocks(list(schema), blocks(False))
    BlockFile(keyed).write_raw_blocks([*schema, ("g", ColumnType.INTEGER)], blocks(True))
    return str(plain), str(keyed)


def expected(keyed_path: str, where, aggs) -> list[dict]:
    df = DataFrame(object()).table(keyed_path)
    if where is not None:
        df = df.filter(where)
    rows = run_query(df.group_by(Col("g")).agg(*aggs()).task)
    return [{k: v for k, v in r.items() if k != "g"} for r in rows]


def whole(engine, plain_path: str, where, aggs) -> DataFrame:
    df = DataFrame(engine).table(plain_path)
    if where is not None:
        df = df.filter(where)
    return df.agg(*aggs())


def all_aggs():
    return [F.sum(Col("i")).alias("si"), F.min(Col("i")).alias("lo_i"), F.max(Col("i")).alias("hi_i"),
            F.avg(Col("i")).alias("avg_i"), F.sum(Col("f")).alias("sf"), F.min(Col("f")).alias("lo_f"),
            F.max(Col("f")).alias("hi_f"), F.avg(Col("f")).alias("avg_f"), F.count().alias("n"),
            F.sum(Col("f") * Col("i")).alias("sfi")]


WHERES = {
    "none": None,
    "last_row_of_a_unit": Col("j") == Lit(sum(UNIT_SIZES[:7]) - 1),          # only the last row of the 65-row unit
    "empties_a_middle_unit": (Col("j") < Lit(sum(UNIT_SIZES[:5]))) | (Col("j") >= Lit(sum(UNIT_SIZES[:6]))),
    "empties_everything": Col("i") > Lit(5000),
    "like_on_a_dictionary": Col("s").like("a%"),
    "all_negative": Col("i") < Lit(-10),
    "all_positive": (Col("i") > Lit(10)) & (Col("f") > Lit(0.5)),
}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cols = make_columns(sum(UNIT_SIZES))
    return write_pair(tmp_path_factory.mktemp("gagg"), "units", cols, UNIT_SIZES)


@pytest.fixture(scope="module")
def wanted(tables):
    """The oracle's rows per WHERE, computed once and shared."""
    return {name: expected(tables[1], cond, all_aggs) for name, cond in WHERES.items()}


@pytest.fixture(scope="module", params=["short_tail", "general"])
def engine(request):
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        e.short_tail_enabled = request.param == "short_tail"
        yield e


# 1 + 3 + 4: every unit size, every WHERE, exact FLOAT folds (values k/64: no flip is allowed at all)
@pytest.mark.parametrize("name", list(WHERES))
def test_unit_sizes_and_where(engine, tables, wanted, name):
    frame = whole(engine, tables[0], WHERES[name], all_aggs)
    rows = frame.collect()
    want = wanted[name]
    assert len(want) == (0 if name == "empties_everything" else 1)
    assert [list(r) for r in rows] == [list(r) for r in want]  # the aggregate columns only, in the order given
    assert assert_rows_match(rows, want, max_ulps=1) == 0
    columns = frame.collect_columns()
    if not want:
        assert columns == {}  # an empty result has no file, hence no columns: what every empty result gives
    else:
        assert list(columns) == [a.name for a in all_aggs()] and all(len(v) == 1 for v in columns.values())
        assert int(columns["n"][0]) == want[0]["n"] and int(columns["lo_i"][0]) == want[0]["lo_i"]
    assert engine.dev.last_scan["tier"] == "scalar"


# 2: one unit over several chunks - the last arriver folds more than one cell row
def test_one_unit_over_several_chunks(tmp_path, monkeypatch):
    from minispark_amd.execution import HipExecutionEngine

    monkeypatch.setenv("HIPSPARK_CHUNK_STEPS", "1")  # 1024 rows per chunk
    sizes = [5000, 3, 2049]
    cols = make_columns(sum(sizes), seed=11)
    plain, keyed = write_pair(tmp_path, "chunks", cols, sizes)
    want = expected(keyed, Col("i") > Lit(-900), all_aggs)
    for short_tail in (True, False):
        with HipExecutionEngine() as e:
            e.short_tail_enabled = short_tail
            rows = whole(e, plain, Col("i") > Lit(-900), all_aggs).collect()
            assert e.dev.last_scan["chunks"] == 5 + 1 + 3 and e.dev.last_scan["chunk_rows"] == 1024
        assert assert_rows_match(rows, want, max_ulps=1) == 0


# 5: random FLOAT values - at most one f32 flip over the whole case list (a condition, not a measurement)
def test_random_floats(tmp_path, engine):
    flips, values = 0, 0
    for seed, sizes in enumerate([[700, 33, 1], [257, 256, 255, 1000], [4096]]):
        rng = np.random.default_rng(100 + seed)
        n = sum(sizes)
        cols = {"i": rng.integers(-50, 50, n).astype(np.int32), "f": rng.normal(0, 1000, n).astype(np.float32),
                "s": ["x"] * n, "j": np.arange(n, dtype=np.int32)}
        plain, keyed = write_pair(tmp_path, f"rand{seed}", cols, sizes)
        for cond in (None, Col("f") > Lit(0.0), Col("i") < Lit(0)):
            want = expected(keyed, cond, all_aggs)
            rows = whole(engine, plain, cond, all_aggs).collect()
            flips += assert_rows_match(rows, want, max_ulps=1)
            values += sum(1 for v in want[0].values() if type(v) is float)
    assert values <= 300
    assert flips <= 1, f"{flips} of {values} FLOAT values differ from the oracle by one f32 ulp"


# 6: two runs on fresh engines give the same bits
def test_two_fresh_engines_give_bitwise_equal_columns(tmp_path):
    from minispark_amd.execution import HipExecutionEngine

    rng = np.random.default_rng(5)
    sizes = [3000, 1, 777]
    n = sum(sizes)
    cols = {"i": rng.integers(-50, 50, n).astype(np.int32), "f": rng.normal(0, 1e4, n).astype(np.float32), "s": ["x"] * n,
            "j": np.arange(n, dtype=np.int32)}
    plain, _ = write_pair(tmp_path, "det", cols, sizes)
    runs = []
    for _ in range(2):
        with HipExecutionEngine() as e:
            runs.append(whole(e, plain, Col("i") != Lit(3), all_aggs).collect_columns())
    assert list(runs[0]) == list(runs[1])
    for name in runs[0]:
        assert np.asarray(runs[0][name]).tobytes() == np.asarray(runs[1][name]).tobytes(), name


# 7: INTEGER overflow raises what the constant-key grouped query raises
def _overflow_tables(folder):
    big = 2_000_000_000
    schema = [("i", ColumnType.INTEGER), ("f", ColumnType.FLOAT), ("s", ColumnType.STRING), ("j", ColumnType.INTEGER)]

    def table(name, values, sizes):
        n = len(values)
        cols = {"i": np.asarray(values, dtype=np.int32), "f": np.zeros(n, dtype=np.float32), "s": ["x"] * n,
                "j": np.arange(n, dtype=np.int32)}
        return write_pair(folder, name, cols, sizes, schema)

    return {"in_unit": table("in_unit", [big, big, 1, 2, 3], [3, 2]),              # unit 0 sums to 4e9 + 1
            "merged": table("merged", [big, 5, big, 7], [2, 2]),                     # each unit fits, their sum does not
            "cancels": table("cancels", [big, big, -big, -big, 9, 1], [5, 1])}       # 4e9 inside the unit, 9 at its end


@pytest.mark.parametrize("name", ["in_unit", "merged", "cancels"])
def test_integer_overflow_is_the_grouped_querys(tmp_path, engine, name):
    plain, keyed = _overflow_tables(tmp_path)[name]
    aggs = lambda: [F.sum(Col("i")).alias("s"), F.count().alias("n")]  # noqa: E731
    grouped = DataFrame(engine).table(keyed).group_by(Col("g")).agg(*aggs())
    frame = whole(engine, plain, None, aggs)
    if name == "cancels":  # 4e9 on the way, 10 at the unit's end: i64 inside the unit, nothing to raise
        assert [{k: v for k, v in r.items() if k != "g"} for r in grouped.collect()] == [{"s": 10, "n": 6}]
        assert frame.collect() == [{"s": 10, "n": 6}]
        return
    with pytest.raises(Exception) as want:
        grouped.collect()
    with pytest.raises(Exception) as got:
        frame.collect()
    assert type(got.value) is type(want.value) and type(got.value).__name__ == "OverflowError"


# 8: sixteen distinct accumulators, INTEGER and FLOAT mixed
def test_sixteen_accumulators(engine, tables, tmp_path):
    def aggs():
        out = []
        for k in range(4):
            out += [F.sum(Col("i") + Lit(k)).alias(f"si{k}"), F.sum(Col("f") * Lit(float(k + 1))).alias(f"sf{k}"),
                    F.min(Col("i") * Lit(k + 1)).alias(f"mi{k}"), F.max(Col("f") + Lit(float(k))).alias(f"mf{k}")]
        return out

    want = expected(tables[1], Col("j") > Lit(2), aggs)
    rows = whole(engine, tables[0], Col("j") > Lit(2), aggs).collect()
    assert len(rows[0]) == 16
    assert assert_rows_match(rows, want, max_ulps=1) == 0
    with pytest.raises(Exception, match="more than 16 distinct aggregates"):
        whole(engine, tables[0], None, lambda: [*aggs(), F.max(Col("j"))]).collect()


# 9: the interpreter (HIPSPARK_JIT=0, read once per process: one child) gives the compiled form's bits
def test_both_evaluator_forms_give_equal_bits(tables, tmp_path):
    out = {}
    for jit in ("1", "0"):
        path = tmp_path / f"jit{jit}.json"
        env = dict(os.environ, HIPSPARK_JIT=jit)
        proc = subprocess.run([sys.executable, str(ROOT / "tests" / "global_agg_worker.py"), "forms", str(path), tables[0]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert proc.returncode == 0, proc.stdout.decode()[-3000:]
        out[jit] = json.loads(path.read_text())
    assert out["1"]["jit_launches"] > 0 and out["0"]["jit_launches"] == 0
    assert out["1"]["rows"] == out["0"]["rows"]  # floats as hex: equal bits
    assert set(out["1"]["rows"]) == set(WHERES)


def test_the_interpreter_matches_the_oracle(tables, wanted, tmp_path):
    path = tmp_path / "interp.json"
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "global_agg_worker.py"), "forms", str(path), tables[0]],
                          env=dict(os.environ, HIPSPARK_JIT="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert proc.returncode == 0, proc.stdout.decode()[-3000:]
    got = json.loads(path.read_text())["rows"]
    for name, want in wanted.items():
        rows = [{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in r.items()} for r in got[name]]
        assert assert_rows_match(rows, want, max_ulps=1) == 0, name


# 10: routes
def test_replay_gives_equal_rows(engine, tables, wanted):
    frame = whole(engine, tables[0], WHERES["all_positive"], all_aggs)
    runs = [frame.collect() for _ in range(3)]  # first run, the recorded run, a replay (where the route records)
    assert runs[0] == runs[1] == runs[2]
    assert assert_rows_match(runs[2], wanted["all_positive"], max_ulps=1) == 0


def test_a_scan_streamed_in_ranges(tables, wanted):
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        e.hbm_budget = 6000  # the table's referenced columns hold ~ 13 KB: at least three ranges
        frame = whole(e, tables[0], WHERES["empties_a_middle_unit"], all_aggs)
        rows = frame.collect()
        assert e.streamed_ranges >= 3
        assert assert_rows_match(rows, wanted["empties_a_middle_unit"], max_ulps=1) == 0
        before = e.streamed_ranges
        assert whole(e, tables[0], WHERES["empties_everything"], all_aggs).collect() == []
        assert e.streamed_ranges > before


USERS = [("user_id", ColumnType.INTEGER), ("w", ColumnType.FLOAT)]
ORDERS = [("user_id", ColumnType.INTEGER), ("price", ColumnType.FLOAT), ("quantity", ColumnType.INTEGER)]


@pytest.fixture(scope="module")
def join_tables(tmp_path_factory):
    """users (unique keys, two blocks) and orders (random FLOAT prices, several keys without a user, three blocks), orders
    also with the constant column g; the expected rows of the three WHEREs, computed once."""
    rng = np.random.default_rng(21)
    folder = tmp_path_factory.mktemp("gagg_join")
    n_users, n_orders = 150, 700
    users = {"user_id": np.arange(n_users, dtype=np.int32), "w": rng.normal(0, 3, n_users).astype(np.float32)}
    orders = {"user_id": rng.integers(0, n_users + 40, n_orders).astype(np.int32),
              "price": rng.normal(50, 400, n_orders).astype(np.float32),
              "quantity": rng.integers(1, 90, n_orders).astype(np.int32)}
    u_path, _ = write_pair(folder, "users", users, [97, 53], USERS)
    o_path, o_keyed = write_pair(folder, "orders", orders, [300, 1, 399], ORDERS)
    want = {}
    for name, cond in JOIN_WHERES.items():
        keyed = joined(object(), u_path, o_keyed)
        if cond is not None:
            keyed = keyed.filter(cond)
        rows = run_query(keyed.group_by(Col("o.g")).agg(*join_aggs()).task)
        want[name] = [{k: v for k, v in r.items() if k not in ("g", "o.g")} for r in rows]
    assert len(want["none"]) == 1 and len(want["positive_prices"]) == 1 and want["nothing"] == []
    return u_path, o_path, want


def joined(eng, users, orders):
    return (DataFrame(eng).table(users).alias("u")
            .join(DataFrame(eng).table(orders).alias("o"), on=Col("u.user_id") == Col("o.user_id"), how="inner"))


def join_aggs():
    return [F.count().alias("n"), F.sum(Col("o.price")).alias("p"), F.max(Col("o.quantity")).alias("q"),
            F.avg(Col("o.price") * Col("u.w")).alias("m"), F.min(Col("u.w")).alias("lo")]


JOIN_WHERES = {"none": None, "positive_prices": Col("o.price") > Lit(0.0), "nothing": Col("o.quantity") > Lit(1000)}


def _join_case(eng, join_tables, name):
    u_path, o_path, want = join_tables
    frame = joined(eng, u_path, o_path)
    if JOIN_WHERES[name] is not None:
        frame = frame.filter(JOIN_WHERES[name])
    rows = frame.agg(*join_aggs()).collect()
    assert [list(r) for r in rows] == [list(r) for r in want[name]]
    return assert_rows_match(rows, want[name], max_ulps=1)


def test_a_join_feeds_the_aggregate(engine, join_tables):
    """The join's materialised rows, units = shuffle partitions, against the oracle's constant-key GROUP BY over the same
    join: 1 ulp per value and at most one flip over the cases (6 FLOAT values)."""
    flips = sum(_join_case(engine, join_tables, name) for name in JOIN_WHERES)
    assert flips <= 1


def test_a_join_with_a_streamed_probe_side_feeds_the_aggregate(join_tables):
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        e.hbm_budget = 3000  # orders' referenced columns hold 8.4 KB: its scan streams in ranges, the join runs resident
        flips = sum(_join_case(e, join_tables, name) for name in JOIN_WHERES)
        assert e.streamed_ranges >= 3 and e.last_probe_route == "resident"
    assert flips <= 1


def test_order_by_limit_and_sql_on_top(engine, tables, wanted):
    want = wanted["like_on_a_dictionary"]
    frame = whole(engine, tables[0], WHERES["like_on_a_dictionary"], all_aggs).order_by(Col("n").desc()).limit(1)
    assert assert_rows_match(frame.collect(), want, max_ulps=1) == 0
    assert whole(engine, tables[0], WHERES["none"], all_aggs).limit(0).collect() == []
    sql = (f"SELECT SUM(i) AS si, MIN(i) AS lo_i, MAX(i) AS hi_i, AVG(i) AS avg_i, SUM(f) AS sf, MIN(f) AS lo_f, "
           f"MAX(f) AS hi_f, AVG(f) AS avg_f, COUNT() AS n, SUM(f * i) AS sfi FROM '{tables[0]}' WHERE s LIKE 'a%';")
    assert assert_rows_match(engine.sql(sql).collect(), want, max_ulps=1) == 0
    assert engine.sql(f"SELECT COUNT() FROM '{tables[0]}';").collect() == [{"count": sum(UNIT_SIZES)}]


# 11: two ranks over gloo on one GPU
def test_two_ranks(tables, wanted, tmp_path):
    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "global_agg_worker.py", "ranks", out, tables[0]])
    got = json.loads(out.read_text())
    for name in ("none", "empties_a_middle_unit", "empties_everything"):
        rows = [{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in r.items()} for r in got[name]]
        assert assert_rows_match(rows, wanted[name], max_ulps=1) == 0, name
