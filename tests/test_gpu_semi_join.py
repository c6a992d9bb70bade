"""LEFT SEMI / LEFT ANTI joins end to end on the GPU.  The model is plain Python over the oracle's rows of the two input
queries (oracle/py_engine.py does not know the task): ``A LEFT SEMI JOIN B ON a.k = b.k`` is ``[row of A if row.k in {b.k}]`` -
A's columns, A's rows, A's order - and the anti join its complement.  Rows are compared exactly; a GROUP BY after the semi
join must have the BITS of the same GROUP BY after the WHERE that names the surviving keys one by one."""

from __future__ import annotations

from datetime import datetime

import pytest

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

PATHS = load_golden("join_group")["paths"]  # 300 orders in blocks of 128 / 128 / 44, 1200 lines
ORDERS, LINEITEM = PATHS["orders"], PATHS["lineitem"]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


@pytest.fixture(scope="module")
def api(engine):
    from minispark_amd.workloads import engine_api

    return engine_api(engine)


def oracle_rows(path):
    from minispark_amd.dataframe import DataFrame
    from oracle.py_engine import run_query

    return run_query(DataFrame(object()).table(path).task)


@pytest.fixture(scope="module")
def orders():
    return oracle_rows(ORDERS)


@pytest.fixture(scope="module")
def lines():
    return oracle_rows(LINEITEM)


def keys_above(lines, quantity):
    return {r["l_orderkey"] for r in lines if r["l_quantity"] > quantity}


def write_table(path, schema, columns, rows_per_block=4):
    from oracle import blockfile

    types = {"INTEGER": blockfile.INTEGER, "STRING": blockfile.STRING, "FLOAT": blockfile.FLOAT, "TIMESTAMP": blockfile.TIMESTAMP}
    blockfile.write_blockfile(path, [(name, types[kind]) for name, kind in schema], columns, rows_per_block)
    return str(path)


def test_the_cardinalities_of_the_golden_tables(orders, lines):
    assert (len(orders), len(lines)) == (300, 1200)
    assert {r["o_orderkey"] for r in orders} <= {r["l_orderkey"] for r in lines}  # every order has a line
    assert len(keys_above(lines, 45)) == 112 and len(keys_above(lines, 49)) == 25
    assert sum(r["o_orderkey"] in keys_above(lines, 45) for r in orders) == 112


# ---- rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["left_semi", "left_anti"])
def test_rows_are_the_python_filter_of_the_left_rows_in_order(engine, api, orders, lines, how):
    C = api.Col
    right = api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 45)
    got = api.DataFrame().table(ORDERS).join(right, on=C("o_orderkey") == C("l_orderkey"), how=how).collect()
    keep = keys_above(lines, 45)
    want = [r for r in orders if (r["o_orderkey"] in keep) == (how == "left_semi")]
    assert len(want) == (112 if how == "left_semi" else 188)
    assert got == want  # the left side's columns, rows and order
    assert engine.dev.last_semi_join["mode"] == "bitmap"


def test_every_order_has_a_line(engine, api, orders):
    C = api.Col
    on = C("o_orderkey") == C("l_orderkey")
    assert api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM), on=on, how="left_semi").collect() == orders
    assert api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM), on=on, how="left_anti").collect() == []


def test_the_api_the_and_form_and_the_sql_text_agree(engine, api, orders, lines):
    C = api.Col
    on = C("o_orderkey") == C("l_orderkey")
    filtered = (api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 45), on=on, how="left_semi")
                .select(C("o_orderkey"), C("o_totalprice")).collect())
    and_form = (api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM), on=on & (C("l_quantity") > 45), how="left_semi")
                .select(C("o_orderkey"), C("o_totalprice")).collect())
    text = engine.sql(f"SELECT o_orderkey, o_totalprice FROM '{ORDERS}' LEFT SEMI JOIN '{LINEITEM}' "
                      "ON o_orderkey = l_orderkey AND l_quantity > 45;").collect()
    keep = keys_above(lines, 45)
    want = [{"o_orderkey": r["o_orderkey"], "o_totalprice": r["o_totalprice"]} for r in orders if r["o_orderkey"] in keep]
    assert filtered == want and and_form == want and text == want
    anti = engine.sql(f"SELECT o.o_orderkey FROM '{ORDERS}' AS o ANTI JOIN '{LINEITEM}' AS l "
                      "ON o.o_orderkey = l.l_orderkey AND l.l_quantity > 45;").collect()
    assert anti == [{"o_orderkey": r["o_orderkey"]} for r in orders if r["o_orderkey"] not in keep]


# ---- float bits ------------------------------------------------------------------------------------------------------------
def test_a_group_by_after_the_semi_join_has_the_bits_of_the_where_form(engine, api, lines):
    """25 surviving keys: GROUP BY o_orderpriority over the semi join against the oracle's run of ORDERS WHERE k = v1 OR k = v2
    ... - the units (file blocks) and the row order are the same, so every FLOAT sum is folded in the same order."""
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions
    from oracle.py_engine import run_query

    C, F = api.Col, api.F
    keep = sorted(keys_above(lines, 49))
    assert len(keep) == 25

    def aggregates(ns, frame):
        return frame.group_by(ns.Col("o_orderpriority")).agg(ns.F.count().alias("n"), ns.F.sum(ns.Col("o_totalprice")).alias("total"),
                                                             ns.F.avg(ns.Col("o_totalprice")).alias("mean"),
                                                             ns.F.max(ns.Col("o_totalprice")).alias("top"))

    right = api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 49)
    got = aggregates(api, api.DataFrame().table(ORDERS).join(right, on=C("o_orderkey") == C("l_orderkey"), how="left_semi")).collect()
    where = Col("o_orderkey") == keep[0]
    for k in keep[1:]:
        where = where | (Col("o_orderkey") == k)

    class plain:  # the oracle's namespace
        pass

    plain.Col, plain.F = Col, Functions
    want = run_query(aggregates(plain, DataFrame(object()).table(ORDERS).filter(where)).task)

    def bits(rows):
        return sorted(tuple(v.hex() if type(v) is float else v for v in r.values()) for r in rows)

    print("semi join:", bits(got))
    print("WHERE form (oracle):", bits(want))
    assert [list(r) for r in got[:1]] == [list(r) for r in want[:1]]  # the same columns
    assert bits(got) == bits(want)
    assert sum(r["n"] for r in got) == 25


# ---- key kinds -------------------------------------------------------------------------------------------------------------
def test_a_dictionary_coded_string_key(engine, api, lines, tmp_path):
    modes = write_table(tmp_path / "modes.bin", [("mode", "STRING")], [["AIR", "TRUCK", "NO SUCH MODE"]])
    C = api.Col
    for how in ("left_semi", "left_anti"):
        got = (api.DataFrame().table(LINEITEM).join(api.DataFrame().table(modes), on=C("l_shipmode") == C("mode"), how=how)
               .select(C("l_orderkey"), C("l_shipmode"), C("l_quantity")).collect())
        want = [{"l_orderkey": r["l_orderkey"], "l_shipmode": r["l_shipmode"], "l_quantity": r["l_quantity"]} for r in lines
                if (r["l_shipmode"] in ("AIR", "TRUCK")) == (how == "left_semi")]
        assert got == want and 0 < len(want) < len(lines)
        assert engine.dev.last_semi_join["mode"] == "global hash table"


def test_a_timestamp_key(engine, api, lines, tmp_path):
    present = sorted({r["l_shipdate"] for r in lines})[:2]
    days = write_table(tmp_path / "days.bin", [("day", "TIMESTAMP")], [[*present, datetime(2031, 5, 6), present[0]]])
    C = api.Col
    for how in ("left_semi", "left_anti"):
        got = (api.DataFrame().table(LINEITEM).join(api.DataFrame().table(days), on=C("day") == C("l_shipdate"), how=how)
               .select(C("l_orderkey"), C("l_shipdate")).collect())
        want = [{"l_orderkey": r["l_orderkey"], "l_shipdate": r["l_shipdate"]} for r in lines
                if (r["l_shipdate"] in present) == (how == "left_semi")]
        assert got == want and 0 < len(want) < len(lines)
        assert engine.dev.last_semi_join["mode"] == "global hash table"


def test_sparse_integer_keys_take_the_hashed_windows(engine, api, tmp_path):
    left_keys = [I32_MIN, -5, 0, 7, 1 << 30, I32_MAX, 12345, -(1 << 30), 7, I32_MIN + 1, I32_MAX - 1, 99]
    right_keys = [I32_MAX, 7, I32_MIN, 8, -(1 << 30) + 1, 7, 100]
    left = write_table(tmp_path / "left.bin", [("k", "INTEGER"), ("tag", "STRING")], [left_keys, [f"row{i}" for i in range(len(left_keys))]])
    right = write_table(tmp_path / "right.bin", [("rk", "INTEGER")], [right_keys])
    C = api.Col
    for how in ("left_semi", "left_anti"):
        got = api.DataFrame().table(left).join(api.DataFrame().table(right), on=C("k") == C("rk"), how=how).collect()
        want = [{"k": k, "tag": f"row{i}"} for i, k in enumerate(left_keys) if (k in right_keys) == (how == "left_semi")]
        assert got == want
        assert engine.dev.last_semi_join["mode"] == "hashed windows"
    # the same right keys without the extremes: a range of 101 slots, the bitmap
    near = write_table(tmp_path / "near.bin", [("rk", "INTEGER")], [[7, 8, 100, 7, 0]])
    got = api.DataFrame().table(left).join(api.DataFrame().table(near), on=C("k") == C("rk"), how="left_semi").collect()
    assert got == [{"k": k, "tag": f"row{i}"} for i, k in enumerate(left_keys) if k in (7, 8, 100, 0)]
    assert engine.dev.last_semi_join["mode"] == "bitmap" and engine.dev.last_semi_join["slots"] == 101


# ---- empty sides and duplicates --------------------------------------------------------------------------------------------
def test_an_empty_right_side(engine, api, orders):
    C = api.Col
    nothing = lambda: api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 1000)  # noqa: E731
    on = C("o_orderkey") == C("l_orderkey")
    assert api.DataFrame().table(ORDERS).join(nothing(), on=on, how="left_semi").collect() == []
    assert api.DataFrame().table(ORDERS).join(nothing(), on=on, how="left_anti").collect() == orders


def test_an_empty_left_side(engine, api):
    C = api.Col
    on = C("o_orderkey") == C("l_orderkey")
    for how in ("left_semi", "left_anti"):
        left = api.DataFrame().table(ORDERS).filter(C("o_totalprice") < 0)
        assert left.join(api.DataFrame().table(LINEITEM), on=on, how=how).collect() == []


def test_duplicates_on_either_side(engine, api, tmp_path):
    left_keys = [3, 1, 3, 2, 3, 9, 1, 4, 4]
    left = write_table(tmp_path / "left.bin", [("k", "INTEGER"), ("v", "FLOAT")], [left_keys, [float(i) / 4 for i in range(9)]],
                       rows_per_block=2)
    right = write_table(tmp_path / "right.bin", [("rk", "INTEGER"), ("w", "INTEGER")], [[3, 3, 3, 4, 7, 3], list(range(6))])
    C = api.Col
    rows = [{"k": k, "v": i / 4} for i, k in enumerate(left_keys)]
    semi = api.DataFrame().table(left).join(api.DataFrame().table(right), on=C("k") == C("rk"), how="left_semi").collect()
    anti = api.DataFrame().table(left).join(api.DataFrame().table(right), on=C("k") == C("rk"), how="left_anti").collect()
    assert semi == [r for r in rows if r["k"] in (3, 4)]  # all copies of a left row are kept; the right side's change nothing
    assert anti == [r for r in rows if r["k"] not in (3, 4)]


# ---- combinations ----------------------------------------------------------------------------------------------------------
def rowset(rows):
    return sorted(tuple(r.values()) for r in rows)


def test_a_semi_join_then_an_inner_join(engine, api, orders, lines):
    C = api.Col
    keep = keys_above(lines, 49)
    on = C("o_orderkey") == C("l_orderkey")
    semi = api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 49), on=on, how="left_semi")
    got = (semi.join(api.DataFrame().table(LINEITEM).alias("l2"), on=C("o_orderkey") == C("l2.l_orderkey"), how="inner")
           .select(C("o_orderkey"), C("o_orderpriority"), C("l2.l_quantity")).collect())
    want = [(o["o_orderkey"], o["o_orderpriority"], li["l_quantity"]) for o in orders if o["o_orderkey"] in keep
            for li in lines if li["l_orderkey"] == o["o_orderkey"]]
    assert list(got[0]) == ["o_orderkey", "o_orderpriority", "l_quantity"]
    assert rowset(got) == sorted(want) and len(want) > 25


def test_an_inner_join_then_an_anti_join(engine, api, orders, lines, tmp_path):
    modes = write_table(tmp_path / "modes.bin", [("mode", "STRING")], [["AIR", "TRUCK", "MAIL", "SHIP"]])
    text = (f"SELECT o_orderkey, l_shipmode, l_quantity FROM '{ORDERS}' JOIN '{LINEITEM}' ON o_orderkey = l_orderkey "
            f"LEFT ANTI JOIN '{modes}' ON l_shipmode = mode WHERE l_quantity > 40;")
    got = engine.sql(text).collect()
    known = {o["o_orderkey"] for o in orders}
    want = [(li["l_orderkey"], li["l_shipmode"], li["l_quantity"]) for li in lines
            if li["l_orderkey"] in known and li["l_shipmode"] not in ("AIR", "TRUCK", "MAIL", "SHIP") and li["l_quantity"] > 40]
    assert rowset(got) == sorted(want) and len(want) > 10


def test_a_group_by_result_as_the_left_side(engine, api, orders, lines):
    C, F = api.Col, api.F
    counted = api.DataFrame().table(LINEITEM).group_by(C("l_orderkey")).agg(F.count().alias("n"), F.max(C("l_quantity")).alias("q"))
    urgent = api.DataFrame().table(ORDERS).filter(C("o_orderpriority") == "1-URGENT")
    got = counted.join(urgent, on=C("l_orderkey") == C("o_orderkey"), how="left_semi").collect()
    keep = {o["o_orderkey"] for o in orders if o["o_orderpriority"] == "1-URGENT"}
    want = {}
    for li in lines:
        if li["l_orderkey"] in keep:
            n, q = want.get(li["l_orderkey"], (0, float("-inf")))
            want[li["l_orderkey"]] = (n + 1, max(q, li["l_quantity"]))
    assert rowset(got) == sorted((k, n, q) for k, (n, q) in want.items()) and len(want) > 10


def test_distinct_order_by_limit_and_a_window_item_on_top(engine, api, orders, lines):
    C, F = api.Col, api.F
    keep = keys_above(lines, 45)
    on = C("o_orderkey") == C("l_orderkey")

    def semi():
        return api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM).filter(C("l_quantity") > 45), on=on, how="left_semi")

    kept = [o for o in orders if o["o_orderkey"] in keep]
    got = semi().select(C("o_orderpriority")).distinct().order_by(C("o_orderpriority").desc()).limit(3).collect()
    assert [r["o_orderpriority"] for r in got] == sorted({o["o_orderpriority"] for o in kept}, reverse=True)[:3]
    text = (f"SELECT o_orderkey, o_orderpriority, ROW_NUMBER() OVER (PARTITION BY o_orderpriority ORDER BY o_orderkey) AS rn "
            f"FROM '{ORDERS}' SEMI JOIN '{LINEITEM}' ON o_orderkey = l_orderkey AND l_quantity > 45 ORDER BY o_orderkey LIMIT 40;")
    got = engine.sql(text).collect()
    rank = {}
    want = []
    for o in sorted(kept, key=lambda o: o["o_orderkey"]):
        rank[o["o_orderpriority"]] = rank.get(o["o_orderpriority"], 0) + 1
        want.append({"o_orderkey": o["o_orderkey"], "o_orderpriority": o["o_orderpriority"], "rn": rank[o["o_orderpriority"]]})
    assert got == want[:40]


# ---- repetition, streaming, ranks ------------------------------------------------------------------------------------------
def test_three_repeated_runs_give_equal_rows(engine, api, orders, lines):
    C, F = api.Col, api.F
    on = (C("o_orderkey") == C("l_orderkey")) & (C("l_quantity") > 45)
    plain = api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM), on=on, how="left_anti")
    grouped = (api.DataFrame().table(ORDERS).join(api.DataFrame().table(LINEITEM), on=on, how="left_semi")
               .group_by(C("o_orderpriority")).agg(F.count().alias("n"), F.sum(C("o_totalprice")).alias("s")))
    for frame in (plain, grouped):
        runs = [frame.collect() for _ in range(3)]  # (the row count is read back: no run is a recorded replay)
        assert runs[0] == runs[1] == runs[2] and runs[0]
    assert len(plain.collect()) == 188


def test_inputs_beyond_the_hbm_budget_give_the_resident_rows(engine, api, orders, lines):
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    def queries(ns):
        C, F = ns.Col, ns.F
        on = (C("o_orderkey") == C("l_orderkey")) & (C("l_quantity") > 45)
        semi = ns.DataFrame().table(ORDERS).join(ns.DataFrame().table(LINEITEM), on=on, how="left_semi")
        anti = ns.DataFrame().table(ORDERS).join(ns.DataFrame().table(LINEITEM), on=on, how="left_anti")
        grouped = (ns.DataFrame().table(ORDERS).join(ns.DataFrame().table(LINEITEM), on=on, how="left_semi")
                   .group_by(ns.Col("o_orderpriority")).agg(F.count().alias("n"), F.sum(C("o_orderkey")).alias("keys"),
                                                            F.max(C("o_orderkey")).alias("last")))
        return semi.collect(), anti.collect(), rowset(grouped.collect())

    resident = queries(api)
    with HipExecutionEngine(device=0) as small:
        small.hbm_budget = 2048  # bytes: both tables stream in several ranges
        streamed = queries(engine_api(small))
        assert small.streamed_ranges >= 4
    assert streamed == resident
    assert len(resident[0]) == 112 and len(resident[1]) == 188


def test_on_ranks_the_join_is_refused_before_any_launch(tmp_path):
    """the one-GPU rehearsal of a multi-rank run (a process group of one rank, as HIPSPARK_FORCE_DIST=1 makes in bench.py)"""
    import torch.distributed as dist

    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        with HipExecutionEngine(device=0) as e:
            e.enable_distributed(dist)
            ns = engine_api(e)
            frame = ns.DataFrame().table(ORDERS).join(ns.DataFrame().table(LINEITEM), on=ns.Col("o_orderkey") == ns.Col("l_orderkey"),
                                                      how="left_semi")
            with pytest.raises(NotImplementedError, match="one rank"):
                frame.collect()
            assert getattr(e.dev, "last_semi_join", None) is None  # nothing ran
    finally:
        dist.destroy_process_group()
