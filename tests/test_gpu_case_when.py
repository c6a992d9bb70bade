"""CASE WHEN on the GPU: HS_OP_SEL through hs_eval in both evaluator forms against numpy.where on the raw cells, the
programs' compiled forms, and engine.sql(...) / the DataFrame API / the stage ABI against the oracle extended by the CPU
model of tests/case_when_model.py - every comparison bit-exact (FLOAT values are k/64, so every f64 sum is exact and no
re-association can move an f32 rounding)."""

from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType
from minispark_amd.dataframe import DataFrame
from minispark_amd.io import BlockFile, StrCol
from minispark_amd.sql import Col, Functions as F, Lit
from oracle.py_engine import run_query
from tests import case_when_model
from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


# ======================================================================================================================
# kernel level: hs_eval through the C ABI
# ======================================================================================================================
@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


def word(op, sp, a=0, b=0, c=0):
    return op | (sp << 8) | (a << 16) | (b << 32) | (c << 48)


def raw_program(words, lits=()):
    p = hs.hs_program()
    p.n_ins, p.n_lit = len(words), len(lits)
    for i, w in enumerate(words):
        p.ins[i] = w
    for i, w in enumerate(lits):
        p.lit[i] = w & 0xFFFFFFFFFFFFFFFF
    return p


F64 = lambda x: int(np.float64(x).view(np.uint64))  # noqa: E731
NAN_A, NAN_B = 0x7FF8000000000001, 0xFFF4DEADBEEF0123  # a quiet and a signalling NaN, payloads that tell them apart
X_CELLS = [1 << 63, F64(-0.0), F64(np.inf), NAN_A, (1 << 63) - 1, F64(1.5), 0, 0xFFFFFFFFFFFFFFFF]
Y_CELLS = [(1 << 63) - 1, F64(0.0), F64(-np.inf), NAN_B, 1 << 63, 7, NAN_A ^ 2, F64(-2.25)]
Z_CELLS = [NAN_B ^ 1, 3, F64(-0.0), 1 << 62, F64(np.inf)]
TRUE_CELLS = [1, 0xFFFFFFFFFFFFFFFF, 1 << 63, 2, 1 << 32]  # every nonzero cell is true, the sign bit alone included
LIT_X, LIT_Y = NAN_B, 1 << 63

LD, LIT, SEL, OUT = hs.OP_LD, hs.OP_LIT, hs.OP_SEL, hs.OP_OUT
# column slots: 0 c, 1 c2, 2 x, 3 y, 4 z.  name -> (program, [expected cells of OUT k as a function of the columns])
PROGRAMS = {
    "sel_at_sp3": (raw_program([word(LD, 0, 0), word(LD, 1, 2), word(LD, 2, 3), word(SEL, 3), word(OUT, 1, 0)]),
                   lambda c, c2, x, y, z: [np.where(c != 0, x, y)]),
    # five cells below the three operands: SEL at sp = HS_MAX_STACK writes cell 5 and leaves cells 0 .. 4 alone
    "sel_at_max_stack": (raw_program([word(LD, 0, 2), word(LD, 1, 3), word(LD, 2, 4), word(LD, 3, 1), word(LD, 4, 3),
                                      word(LD, 5, 0), word(LD, 6, 2), word(LD, 7, 3), word(SEL, 8),
                                      word(OUT, 6, 0), word(OUT, 5, 1), word(OUT, 4, 2), word(OUT, 3, 3), word(OUT, 2, 4),
                                      word(OUT, 1, 5)]),
                         lambda c, c2, x, y, z: [np.where(c != 0, x, y), y, c2, z, y, x]),
    # a SEL as the THEN value of another, and a SEL as the condition of another
    "sel_feeds_sel": (raw_program([word(LD, 0, 0), word(LD, 1, 1), word(LD, 2, 2), word(LD, 3, 3), word(SEL, 4), word(LD, 2, 4),
                                   word(SEL, 3), word(OUT, 1, 0),
                                   word(LD, 0, 0), word(LD, 1, 1), word(LD, 2, 0), word(SEL, 3), word(LD, 1, 4), word(LD, 2, 2),
                                   word(SEL, 3), word(OUT, 1, 1)]),
                      lambda c, c2, x, y, z: [np.where(c != 0, np.where(c2 != 0, x, y), z),
                                              np.where(np.where(c != 0, c2, c) != 0, z, x)]),
    "literal_branches": (raw_program([word(LD, 0, 0), word(LIT, 1, 0), word(LIT, 2, 1), word(SEL, 3), word(OUT, 1, 0),
                                      word(LIT, 0, 2), word(LIT, 1, 0), word(LIT, 2, 1), word(SEL, 3), word(OUT, 1, 1),
                                      word(LIT, 0, 3), word(LIT, 1, 0), word(LIT, 2, 1), word(SEL, 3), word(OUT, 1, 2)],
                                     [LIT_X, LIT_Y, 0, 1 << 63]),
                         lambda c, c2, x, y, z: [np.where(c != 0, np.uint64(LIT_X), np.uint64(LIT_Y)),
                                                 np.full(len(c), LIT_Y, np.uint64), np.full(len(c), LIT_X, np.uint64)]),
}
ROW_COUNTS = [1, 3, 4, 5, 255, 1023, 1025, 4099]
# (rows, first condition): the alternation starts at 0, so the single row of n = 1 takes ELSE; (1, 1) is the one lane taking THEN
KERNEL_CASES = [(n, 0) for n in ROW_COUNTS] + [(1, 1)]


def cycle(cells, n, shift=0):
    return np.array([cells[(i + shift) % len(cells)] for i in range(n)], dtype=np.uint64)


def conditions(n, first=0):
    """alternating from ``first``, then all true, then all false - each third of the rows (n < 3: alternating only)"""
    c = np.array([(i + first) & 1 for i in range(n)], dtype=np.uint64)
    if n >= 3:
        c[n // 3: 2 * n // 3] = cycle(TRUE_CELLS, 2 * n // 3 - n // 3)
        c[2 * n // 3:] = 0
    return c


@pytest.fixture(scope="module")
def kernel_inputs(dev):
    """host columns and their device copies per row count, uploaded once"""
    out = {}
    for n, first in KERNEL_CASES:
        host = [conditions(n, first), cycle([0, 1, 1, 0, 1 << 63], n, first), cycle(X_CELLS, n), cycle(Y_CELLS, n, 3),
                cycle(Z_CELLS, n, 1)]
        out[n, first] = (host, [dev.fixed_col(hs.I64, h.view(np.int64)) for h in host])
    return out


@pytest.mark.parametrize("jit", [1, 0], ids=["compiled", "interpreter"])
@pytest.mark.parametrize("n,first", KERNEL_CASES, ids=[f"{n}" if not first else f"{n}-then" for n, first in KERNEL_CASES])
def test_sel_moves_raw_cells_in_both_evaluator_forms(dev, kernel_inputs, n, first, jit):
    import torch

    host, cols = kernel_inputs[n, first]
    arr = (hs.hs_col * len(cols))(*[c.as_hs() for c in cols])
    stats = (C.c_int32 * 3)()
    dev.lib.hs_jit_stats(stats)
    launched, failed = stats[1], stats[2]
    dev.reset_flags()
    dev.lib.hs_jit_set_enabled(jit)
    try:
        for name, (prog, expect) in PROGRAMS.items():
            want = expect(*host)
            outs = [dev.empty(n, torch.int64) for _ in want]
            for o in outs:
                o.fill_(0x5A5A5A5A5A5A5A5A)
            ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            kinds = (C.c_int32 * len(outs))(*[hs.I64] * len(outs))
            hs.check(dev.lib.hs_eval(dev.stream, arr, len(cols), C.byref(prog), None, n, None, ptrs, kinds, len(outs),
                                     dev.flags.data_ptr()), "hs_eval")
            for k, (o, w) in enumerate(zip(outs, want)):
                got = o.cpu().numpy().view(np.uint64)
                assert got.tobytes() == np.asarray(w, dtype=np.uint64).tobytes(), (name, k, n, jit)
        assert dev.read_flags() == 0  # SEL raises nothing; HS_FLAG_BAD_PROGRAM here = the opcode is unknown
        dev.lib.hs_jit_stats(stats)
        assert stats[2] == failed, dev.lib.hs_jit_last_log()
        assert (stats[1] - launched == len(PROGRAMS)) if jit else (stats[1] == launched), "not the evaluator form asked for"
    finally:
        dev.lib.hs_jit_set_enabled(1)
        dev.reset_flags()


def test_programs_with_sel_compile():
    """hs_jit_compile_check / _scalar / _eval: the translator covers SEL (the interpreter fallback would make every parity
    test pass while the hot path is not the new one)."""
    from tests.test_case_when_cpu import check_sel_programs_compile

    check_sel_programs_compile()


# ======================================================================================================================
# engine level
# ======================================================================================================================
SCHEMA = [("k", ColumnType.INTEGER), ("i", ColumnType.INTEGER), ("b", ColumnType.INTEGER), ("f", ColumnType.FLOAT),
          ("s", ColumnType.STRING), ("j", ColumnType.INTEGER)]
PRIORITIES = ["1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"]
SIZES = {"one": [1], "two_blocks": [512, 513], "six_blocks": [1000, 1, 999, 1500, 777, 723]}  # 1, 1025 and 5000 rows


def make_columns(n: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 5, n).astype(np.int32)
    pick = rng.integers(0, 5, n)
    pick[k == 3] = rng.integers(2, 5, int((k == 3).sum()))  # group 3: no row is URGENT / HIGH
    pick[k == 4] = 0                                        # group 4: every row is URGENT
    b = rng.integers(1, 60, n).astype(np.int32) * np.where(rng.random(n) < 0.5, 1, -1).astype(np.int32)
    return {"k": k, "i": rng.integers(-1000, 1000, n).astype(np.int32), "b": b,
            "f": (rng.integers(-(1 << 20) + 1, 1 << 20, n) / 64.0).astype(np.float32),  # k/64: f64 sums are exact
            "s": [PRIORITIES[p] for p in pick], "j": np.arange(n, dtype=np.int32)}


def write_pair(folder: Path, name: str, cols: dict, sizes: list[int], schema=SCHEMA) -> tuple[str, str]:
    """The table, and the table with a constant INTEGER column g appended (same block cuts): GROUP BY g there is what an
    aggregate without GROUP BY is compared with."""
    folder.mkdir(parents=True, exist_ok=True)

    def blocks(with_g: bool):
        lo = 0
        for size in sizes:
            part = [StrCol.from_strings(list(cols[c][lo: lo + size])) if t == ColumnType.STRING else np.asarray(cols[c][lo: lo + size])
                    for c, t in schema]
            if with_g:
                part.append(np.full(size, 7, dtype=np.int32))
            lo += size
            yield part

    plain, keyed = folder / f"{name}.bin", folder / f"{name}_g.bin"
    BlockFile(plain).write_raw_blocks(list(schema), blocks(False))
    BlockFile(keyed).write_raw_blocks([*schema, ("g", ColumnType.INTEGER)], blocks(True))
    return str(plain), str(keyed)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    folder = tmp_path_factory.mktemp("case_when")
    return {name: write_pair(folder, name, make_columns(sum(sizes), 40 + len(sizes)), sizes) for name, sizes in SIZES.items()}


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


def T(eng, path):
    return DataFrame(eng).table(path)


# ---- the queries: name -> text with {t} for the table ------------------------------------------------------------------
GROUPED_SQL = ("SELECT k, SUM(CASE WHEN s = '1-URGENT' OR s = '2-HIGH' THEN 1 ELSE 0 END) AS high_line_count, "
               "SUM(CASE WHEN s != '1-URGENT' AND s != '2-HIGH' THEN 1 ELSE 0 END) AS low_line_count, "
               "SUM(CASE WHEN s LIKE '1%' THEN f ELSE 0 END) AS urgent_f, AVG(CASE WHEN i > 0 THEN f ELSE i END) AS m, "
               "MIN(CASE WHEN i > 0 THEN i ELSE b END) AS lo, MAX(CASE WHEN s = '5-LOW' THEN f ELSE 0 - f END) AS hi, "
               "COUNT() AS n FROM '{t}' GROUP BY k;")
KEYLESS_AGGS = ("SUM(CASE WHEN s = '1-URGENT' THEN 1 ELSE 0 END) AS u, SUM(CASE WHEN i > 0 THEN f ELSE 0 END) AS pf, "
                "MIN(CASE WHEN b > 0 THEN i ELSE 0 - i END) AS lo, MAX(CASE WHEN s LIKE '%H' THEN f ELSE i END) AS hi, "
                "AVG(CASE WHEN i > b THEN i ELSE b END) AS m, COUNT() AS n")
KEYLESS_SQL = "SELECT " + KEYLESS_AGGS + " FROM '{t}' WHERE j != 3;"
KEYLESS_AS_GROUPED_SQL = "SELECT g, " + KEYLESS_AGGS + " FROM '{t}' WHERE j != 3 GROUP BY g;"
SELECT_SQL = ("SELECT j, CASE WHEN i > b THEN i ELSE b END AS m, CASE WHEN s LIKE '%H' THEN f ELSE i END AS x, "
              "1 + CASE WHEN i > 0 THEN 1 WHEN i < 0 THEN 0 - 1 ELSE 0 END AS sg, "
              "CASE WHEN CASE WHEN b > 0 THEN i ELSE 0 - i END > 100 THEN f * 2 ELSE f END AS nested FROM '{t}';")
WHERE_SQL = "SELECT j, i, b FROM '{t}' WHERE CASE WHEN i > 0 THEN i ELSE b END > 5 AND j != 1;"
WHERE_GROUPED_SQL = ("SELECT k, COUNT() AS n, SUM(f) AS sf FROM '{t}' WHERE 2 * CASE WHEN s = '3-MEDIUM' THEN i ELSE b END > 10 "
                     "GROUP BY k;")
MULTI_WHEN_SQL = ("SELECT k, SUM(CASE WHEN i < -500 THEN 1 WHEN i < 0 THEN 20 WHEN i < 500 THEN 300 ELSE 4000 END) AS buckets, "
                  "SUM(CASE WHEN s = '1-URGENT' THEN f WHEN s = '2-HIGH' THEN i WHEN s = '5-LOW' THEN 0 - f ELSE 0 END) AS mixed "
                  "FROM '{t}' GROUP BY k;")
ORDER_SQL = "SELECT j, CASE WHEN i > b THEN i ELSE b END AS m FROM '{t}' ORDER BY m DESC, j LIMIT 9;"
QUERIES = {"grouped": GROUPED_SQL, "select": SELECT_SQL, "where": WHERE_SQL, "where_grouped": WHERE_GROUPED_SQL,
           "multi_when": MULTI_WHEN_SQL}


def model_rows(monkeypatch, text: str) -> list[dict]:
    from minispark_amd.parser import parse_sql

    case_when_model.install(monkeypatch)
    return run_query(parse_sql(text, object()).task)


@pytest.fixture(scope="module")
def wanted(tables):
    """The model's rows of every query on every table, computed once and shared (the oracle's compile_expr is patched for
    the computation only)."""
    mp = pytest.MonkeyPatch()
    try:
        out = {(q, name): model_rows(mp, text.format(t=plain)) for q, text in QUERIES.items() for name, (plain, _) in tables.items()}
        for name, (_, keyed) in tables.items():
            rows = model_rows(mp, KEYLESS_AS_GROUPED_SQL.format(t=keyed))
            out[("keyless", name)] = [{k: v for k, v in r.items() if k != "g"} for r in rows]
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("name", list(SIZES))
@pytest.mark.parametrize("query", list(QUERIES))
def test_sql_against_the_model(engine, tables, wanted, query, name):
    rows = engine.sql(QUERIES[query].format(t=tables[name][0])).collect()
    want = wanted[(query, name)]
    assert [list(r) for r in rows[:1]] == [list(r) for r in want[:1]]
    assert assert_rows_match(rows, want) == 0  # max_ulps = 0: equal bits
    if query in ("select", "where") or name != "one":
        assert len(want) > 0
    if query == "select":
        assert len(want) == sum(SIZES[name])


def test_the_grouped_query_covers_a_group_that_never_and_one_that_always_takes_then(wanted):
    by_key = {r["k"]: r for r in wanted[("grouped", "six_blocks")]}
    assert sorted(by_key) == [0, 1, 2, 3, 4]
    assert by_key[3]["high_line_count"] == 0 and by_key[3]["low_line_count"] == by_key[3]["n"] > 0
    assert by_key[4]["high_line_count"] == by_key[4]["n"] > 0 and by_key[4]["low_line_count"] == 0
    assert all(0 < by_key[k]["high_line_count"] < by_key[k]["n"] for k in (0, 1, 2))


@pytest.mark.parametrize("name", list(SIZES))
def test_keyless_aggregates_of_a_case(engine, tables, wanted, name):
    rows = engine.sql(KEYLESS_SQL.format(t=tables[name][0])).collect()
    assert engine.dev.last_scan["tier"] == "scalar"
    assert len(rows) == 1 and assert_rows_match(rows, wanted[("keyless", name)]) == 0


def test_the_api_builds_what_the_text_builds(engine, tables, wanted):
    """Functions.when / .otherwise with FLOAT literals (the SQL grammar's numbers are integers) and an all-literal CASE."""
    plain = tables["six_blocks"][0]

    def frame(eng):
        urgent = (Col("s") == "1-URGENT") | (Col("s") == "2-HIGH")
        return T(eng, plain).group_by(Col("k")).agg(
            F.sum(F.when(urgent, 1).otherwise(0)).alias("high"), F.sum(F.when(Col("i") > 0, Col("f")).otherwise(0.0)).alias("pf"),
            F.sum(F.when(Col("f") * 0.5, 1).otherwise(0)).alias("truthy"), F.sum(F.when(Lit(0), 5).otherwise(7)).alias("sevens"),
            F.max(F.when(Col("i") > 0, 0.25).otherwise(-0.0)).alias("zero"))

    mp = pytest.MonkeyPatch()
    try:
        case_when_model.install(mp)
        want = run_query(frame(object()).task)
    finally:
        mp.undo()
    rows = frame(engine).collect()
    assert assert_rows_match(rows, want) == 0
    assert {r["k"]: r["high"] for r in rows} == {r["k"]: r["high_line_count"] for r in wanted[("grouped", "six_blocks")]}
    assert all(r["sevens"] % 7 == 0 and r["sevens"] > 0 for r in rows)


def test_order_by_over_a_case_alias(engine, tables, monkeypatch):
    plain = tables["six_blocks"][0]
    unsorted = model_rows(monkeypatch, ORDER_SQL.format(t=plain).replace(" ORDER BY m DESC, j LIMIT 9", ""))
    want = sorted(unsorted, key=lambda r: (-r["m"], r["j"]))[:9]  # j is unique: the order is total
    assert engine.sql(ORDER_SQL.format(t=plain)).collect() == want


USERS = [("user_id", ColumnType.INTEGER), ("w", ColumnType.FLOAT), ("grp", ColumnType.INTEGER)]
ORDERS = [("user_id", ColumnType.INTEGER), ("price", ColumnType.FLOAT), ("quantity", ColumnType.INTEGER)]


def test_a_case_over_a_joins_output_feeds_a_group_by(engine, tmp_path, monkeypatch):
    rng = np.random.default_rng(21)
    n_users, n_orders = 150, 700
    users = {"user_id": np.arange(n_users, dtype=np.int32), "w": (rng.integers(-4000, 4000, n_users) / 64.0).astype(np.float32),
             "grp": rng.integers(0, 6, n_users).astype(np.int32)}
    orders = {"user_id": rng.integers(0, n_users + 40, n_orders).astype(np.int32),
              "price": (rng.integers(-4000, 4000, n_orders) / 64.0).astype(np.float32),
              "quantity": rng.integers(1, 90, n_orders).astype(np.int32)}
    u_path, _ = write_pair(tmp_path, "users", users, [97, 53], USERS)
    o_path, _ = write_pair(tmp_path, "orders", orders, [300, 1, 399], ORDERS)

    def frame(eng):
        joined = (T(eng, u_path).alias("u").join(T(eng, o_path).alias("o"), on=Col("u.user_id") == Col("o.user_id"), how="inner"))
        return joined.group_by(Col("u.grp")).agg(
            F.sum(F.when(Col("o.price") > Col("u.w"), Col("o.price")).otherwise(0)).alias("above"),
            F.sum(F.when(Col("o.quantity") > 40, 1).otherwise(0)).alias("big"),
            F.min(F.when(Col("o.quantity") > 40, Col("u.w")).otherwise(Col("o.quantity"))).alias("lo"), F.count().alias("n"))

    case_when_model.install(monkeypatch)
    want = run_query(frame(object()).task)
    assert len(want) == 6
    assert assert_rows_match(frame(engine).collect(), want) == 0


# ---- the eager rule -------------------------------------------------------------------------------------------------------
def test_an_error_in_the_branch_not_taken_is_raised(engine, tmp_path, monkeypatch):
    """CASE WHEN b != 0 THEN i / b ELSE 0.0 END over a table with one b = 0 row raises what the plain i / b raises there:
    both branches are evaluated, then one is chosen.  An error the engine reports through its flags."""
    cols = make_columns(40, 3)
    cols["b"][17] = 0
    plain, _ = write_pair(tmp_path, "zero", cols, [25, 15])
    guarded = F.when(Col("b") != 0, Col("i") / Col("b")).otherwise(0.0)
    with pytest.raises(Exception) as plain_error:
        T(engine, plain).select(Col("j"), (Col("i") / Col("b")).alias("q")).collect()
    assert type(plain_error.value) is ZeroDivisionError
    for build in (lambda eng: T(eng, plain).select(Col("j"), guarded.alias("q")),
                  lambda eng: T(eng, plain).group_by(Col("k")).agg(F.sum(guarded).alias("q")),
                  lambda eng: T(eng, plain).agg(F.sum(guarded).alias("q"))):
        with pytest.raises(Exception) as got:
            build(engine).collect()
        assert type(got.value) is type(plain_error.value) and str(got.value) == str(plain_error.value)
    with pytest.raises(Exception) as got:
        engine.sql(f"SELECT j, CASE WHEN b != 0 THEN i / b ELSE 0 END AS q FROM '{plain}';").collect()
    assert type(got.value) is ZeroDivisionError
    case_when_model.install(monkeypatch)
    with pytest.raises(ZeroDivisionError):
        run_query(T(object(), plain).select(Col("j"), guarded.alias("q")).task)
    # a row the WHERE drops is not evaluated at all: nothing to raise
    kept = T(engine, plain).filter(Col("b") != 0).select(Col("j"), guarded.alias("q"))
    want = run_query(T(object(), plain).filter(Col("b") != 0).select(Col("j"), guarded.alias("q")).task)
    assert len(want) == 39 and assert_rows_match(kept.collect(), want) == 0


# ---- the stage ABI --------------------------------------------------------------------------------------------------------
def test_scan_and_group_by_with_a_case_argument_through_the_stage_abi(engine, tables, monkeypatch):
    from minispark_amd.stage import NativeEngine, NativeStage

    plain = tables["six_blocks"][0]

    def frame(eng):
        return T(eng, plain).filter(Col("j") != 5).group_by(Col("k")).agg(
            F.sum(F.when(Col("i") > Col("b"), Col("f")).otherwise(0)).alias("pf"), F.sum(F.when(Col("i") > 0, 1).otherwise(0)).alias("pos"),
            F.avg(F.when(Col("b") > 0, Col("i")).otherwise(Col("f"))).alias("m"), F.max(F.when(Col("i") > 0, Col("i")).otherwise(Col("b"))).alias("hi"),
            F.count().alias("n"))

    case_when_model.install(monkeypatch)
    want = run_query(frame(object()).task)
    from_engine = frame(engine).collect()
    with NativeEngine(0) as native:
        stage = NativeStage(native, frame(object()).task)
        for _ in range(3):  # first run, recorded run, a replay
            rows = stage.run()
            assert assert_rows_match(rows, from_engine) == 0
        stage.close()
    assert assert_rows_match(from_engine, want) == 0


# ---- the other evaluator form and the undictionaried route, each in one child process ------------------------------------------
def run_worker(tmp_path, tables, **env):
    out = tmp_path / ("worker_" + "_".join(f"{k}{v}" for k, v in env.items()) + ".json")
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "case_when_worker.py"), str(out), tables["six_blocks"][0]],
                          env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert proc.returncode == 0, proc.stdout.decode()[-3000:]
    return json.loads(out.read_text())


def unhex(rows):
    return [{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in r.items()} for r in rows]


def hexed(rows):
    return [{k: (v.hex() if type(v) is float else v) for k, v in r.items()} for r in rows]


def test_the_interpreter_returns_the_compiled_forms_bits(engine, tables, wanted, tmp_path):
    stats = (C.c_int32 * 3)()
    engine.dev._raw_lib.hs_jit_stats(stats)
    before, failed = stats[1], stats[2]
    plain = tables["six_blocks"][0]
    compiled = {"grouped": engine.sql(GROUPED_SQL.format(t=plain)).collect(), "keyless": engine.sql(KEYLESS_SQL.format(t=plain)).collect()}
    engine.dev._raw_lib.hs_jit_stats(stats)
    assert stats[1] > before and stats[2] == failed, "the compiled form did not run in this process"
    got = run_worker(tmp_path, tables, HIPSPARK_JIT="0")
    assert got["jit_launches"] == 0 and got["dict_enabled"] is True
    for name in ("grouped", "keyless"):
        key = lambda r: json.dumps(r, sort_keys=True)  # noqa: E731
        assert sorted(got[name], key=key) == sorted(hexed(compiled[name]), key=key), name  # floats as hex: equal bits
        assert assert_rows_match(unhex(got[name]), wanted[(name, "six_blocks")]) == 0


def test_without_dictionary_coding_the_string_conditions_read_the_bytes(tables, wanted, tmp_path):
    got = run_worker(tmp_path, tables, HIPSPARK_DICT="0")
    assert got["dict_enabled"] is False and got["jit_launches"] > 0
    for name in ("grouped", "keyless"):
        assert assert_rows_match(unhex(got[name]), wanted[(name, "six_blocks")]) == 0
