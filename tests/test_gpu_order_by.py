"""ORDER BY / LIMIT on the GPU.  Kernel level: Device.order_by (hs_order_by) must return exactly the row list of Python's
stable sort - every column type, both directions, several keys, ties, LIMIT cuts through ties.  End to end: queries over
the committed golden tables, through the DataFrame API and through engine.sql, against oracle/py_engine.py's rows of the
same query without its ORDER BY, sorted in Python by the keys."""

from __future__ import annotations

import json

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, f32, f32_ulps, load_golden
from tests.queries import case_by_name
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

RX_TILE = 8192  # rows of one partition-pass workgroup (csrc/hs_radix.hip)
BIG = 3 * RX_TILE + 17


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- kernel level -------------------------------------------------------------------------------------------------------
def ref_perm(n, keys, limit=None):
    """Python's stable sort: keys = [(values, ascending)], the first the most significant."""
    perm = list(range(n))
    for values, ascending in reversed(keys):
        perm.sort(key=lambda i: values[i], reverse=not ascending)  # noqa: B023 - stable also when reversed
    return perm if limit is None else perm[:limit]


def upload(dev, values, col_type):
    from minispark_amd.io import StrCol

    if col_type == T.STRING:  # the column format holds bytes: UTF-8 here (StrCol.from_strings takes ASCII only)
        raw = [v.encode("utf-8") for v in values]
        data = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        return dev.upload_raw(StrCol(np.array([len(b) for b in raw], dtype=np.uint8), data), T.STRING)
    dtype = {T.INTEGER: np.int32, T.FLOAT: np.float32, T.TIMESTAMP: np.int64}[col_type]
    return dev.upload_raw(np.asarray(values, dtype=dtype), col_type)


def device_perm(dev, columns, directions, limit=None, cols=None):
    """columns = [(values, ColumnType)] -> the row list of Device.order_by over all of them as keys."""
    from minispark_amd.device import DBatch

    n = len(columns[0][0])
    cols = cols or [upload(dev, v, t) for v, t in columns]
    batch = DBatch([(f"c{i}", t) for i, (_, t) in enumerate(columns)], cols, n)
    perm, count = dev.order_by(batch, [(i, asc) for i, asc in enumerate(directions)], limit)
    assert perm.numel() == count
    return perm.cpu().tolist()


def py_values(values, col_type):
    if col_type == T.FLOAT:
        return [float(v) for v in np.asarray(values, dtype=np.float32)]
    return [int(v) for v in values] if col_type != T.STRING else list(values)


def check(dev, columns, directions, limit=None):
    n = len(columns[0][0])
    want = ref_perm(n, [(py_values(v, t), asc) for (v, t), asc in zip(columns, directions)], limit)
    assert device_perm(dev, columns, directions, limit) == want


def i32_values(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-2**31, 2**31, n, dtype=np.int64)
    special = [-2**31, -1, 0, 2**31 - 1]
    for j, s in enumerate(special * 2):
        v[(j * 7919) % n] = s
    return v.astype(np.int32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, RX_TILE - 1, RX_TILE, RX_TILE + 1, BIG])
def test_i32_keys_at_every_tile_boundary(dev, n):
    rng = np.random.default_rng(n)
    check(dev, [(i32_values(n, n), T.INTEGER)], [True])
    check(dev, [(rng.integers(-1, 2, n), T.INTEGER)], [True])      # 3 distinct values: ties keep their input order
    check(dev, [(np.full(n, -77), T.INTEGER)], [True])             # constant: every pass is skipped
    check(dev, [(i32_values(n, n + 1), T.INTEGER)], [False])
    check(dev, [(rng.integers(-1, 2, n), T.INTEGER)], [False])     # descending and still stable


F32_SPECIAL = [-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.1754942e-38, 1.0, 3.4e38, np.inf]


def test_f32_keys_order_like_python_floats(dev):
    rng = np.random.default_rng(5)
    n = RX_TILE + 1
    v = rng.normal(0, 1e3, n).astype(np.float32)
    v[rng.integers(0, n, 400)] = rng.choice(np.asarray(F32_SPECIAL, dtype=np.float32), 400)
    tie = rng.integers(0, 3, n)
    check(dev, [(v, T.FLOAT)], [True])
    check(dev, [(v, T.FLOAT)], [False])
    check(dev, [(v, T.FLOAT), (tie, T.INTEGER)], [True, True])
    # -0.0 == +0.0 in Python: the second key decides between them
    f, i = [0.0, -0.0, -0.0, 0.0, 1.0, -1.0], [1, 2, 0, 3, 0, 0]
    assert device_perm(dev, [(f, T.FLOAT), (i, T.INTEGER)], [True, True]) == [5, 2, 0, 1, 3, 4]
    check(dev, [(f, T.FLOAT), (i, T.INTEGER)], [False, True])


def test_timestamp_keys_use_all_64_bits(dev):
    rng = np.random.default_rng(6)
    n = RX_TILE + 65
    v = rng.integers(-2**40, 2**40, n, dtype=np.int64)
    v[::5] = (rng.integers(-128, 128, len(v[::5]), dtype=np.int64) << 56) + 5   # differ in the top byte only
    v[1::7] = rng.integers(2**32, 2**33, len(v[1::7]), dtype=np.int64)
    v[3] = -2**63
    v[4] = 2**63 - 1
    check(dev, [(v, T.TIMESTAMP)], [True])
    check(dev, [(v, T.TIMESTAMP)], [False])
    check(dev, [(np.full(n, 1_700_000_000) + rng.integers(0, 200, n), T.TIMESTAMP)], [True])  # six constant bytes


def string_pool():
    pool = ["", "a", "b", "abcdefg", "abcdefgh", "abcdefghi", "abcdefghijklmnop", "abcdefghijklmnopq", "x" * 255,
            "x" * 254, "x" * 254 + "y", "ab", "abc", "abd", "ab\x00", "ab\x00\x00", "ab\x01", "\x7f", "é", "éa", "ü", "€", "€uro",
            "日本", "日本語", "z", "zz", "Z", "abcdefgé", "abcdefgh€"]
    pool += ["k" * 16 + c for c in "abc"] + ["k" * 17, "k" * 8 + "é" * 3]
    assert {len(s.encode()) for s in pool} >= {0, 1, 7, 8, 9, 16, 17, 255}
    return pool


def test_string_keys_order_like_python_str(dev):
    rng = np.random.default_rng(7)
    pool = string_pool()
    n = RX_TILE + 3
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    check(dev, [(words, T.STRING)], [True])
    check(dev, [(words, T.STRING)], [False])
    check(dev, [(pool, T.STRING)], [True])  # few rows: one string each
    nums = rng.integers(-5, 5, n)
    check(dev, [(words, T.STRING), (nums, T.INTEGER)], [True, False])
    fixed = ["%04d-%s-é" % (j % 97, "ab"[j % 2] * 3) for j in rng.integers(0, 10_000, n)]  # 11 bytes each
    assert len({len(s.encode()) for s in fixed}) == 1
    check(dev, [(fixed, T.STRING)], [True])
    check(dev, [(fixed, T.STRING), (nums, T.INTEGER)], [False, True])


def test_dictionary_coded_string_key_orders_by_its_strings(dev):
    rng = np.random.default_rng(8)
    pool = string_pool()
    n = 5000
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    plain = upload(dev, words, T.STRING)
    coded = dev.dict_encode(plain)
    assert coded is not None and coded.dict is not None
    for ascending in (True, False):
        want = ref_perm(n, [(words, ascending)])
        assert device_perm(dev, [(words, T.STRING)], [ascending], cols=[plain]) == want
        assert device_perm(dev, [(words, T.STRING)], [ascending], cols=[coded]) == want
    # a dictionary that is not sorted is decoded, not trusted
    import dataclasses

    shuffled = dataclasses.replace(coded, dict=tuple(reversed(coded.dict)), plain=None)
    decoded_words = [shuffled.dict[coded.dict.index(w.encode())].decode() for w in words]
    assert device_perm(dev, [(decoded_words, T.STRING)], [True], cols=[shuffled]) == ref_perm(n, [(decoded_words, True)])


def test_several_keys_and_mixed_directions(dev):
    rng = np.random.default_rng(9)
    n = RX_TILE + 1
    a, b = rng.integers(-3, 3, n), rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    check(dev, [(a, T.INTEGER), (b, T.INTEGER)], [True, True])       # two I32 keys share one word
    check(dev, [(a, T.INTEGER), (b, T.INTEGER)], [False, True])
    check(dev, [(a, T.INTEGER), (a[::-1].copy(), T.INTEGER)], [True, False])
    ts = rng.integers(0, 4, n).astype(np.int64) << 40
    f = rng.choice(np.asarray(F32_SPECIAL, dtype=np.float32), n)
    pool = string_pool()
    words = [pool[j] for j in rng.integers(0, 6, n)]
    check(dev, [(ts, T.TIMESTAMP), (f, T.FLOAT), (words, T.STRING)], [False, True, False])
    check(dev, [(words, T.STRING), (f, T.FLOAT), (ts, T.TIMESTAMP)], [True, False, True])


LIMITS = [0, 1, 10, BIG - 1, BIG, BIG + 5]


@pytest.mark.parametrize("limit", LIMITS)
def test_limit_is_the_head_of_the_full_stable_sort(dev, limit):
    rng = np.random.default_rng(10)
    three = rng.integers(-1, 2, BIG)
    check(dev, [(three, T.INTEGER)], [True], limit)             # ties straddle the cut
    check(dev, [(three, T.INTEGER)], [False], limit)
    check(dev, [(np.full(BIG, 5), T.INTEGER)], [True], limit)   # constant: the first rows as they stand
    wide = i32_values(BIG, 11)
    check(dev, [(wide, T.INTEGER), (three, T.INTEGER)], [True, False], limit)


@pytest.mark.parametrize("limit", [None, *LIMITS])
def test_a_lazy_batch_is_ordered_up_to_its_device_row_count(dev, limit):
    import torch

    from minispark_amd.device import DBatch

    rows = BIG - 4000  # what the device says; the buffers hold BIG rows
    values = i32_values(BIG, 12) % 1000
    col = upload(dev, values, T.INTEGER)
    batch = DBatch([("c0", T.INTEGER)], [col], BIG, None, torch.tensor([rows], dtype=torch.int64, device=dev.device))
    perm, count = dev.order_by(batch, [(0, False)], limit)
    want = ref_perm(rows, [([int(v) for v in values[:rows]], False)], limit)
    assert count == len(want) and perm.cpu().tolist() == want


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


def oracle_rows(frame):
    from oracle.py_engine import run_query

    return run_query(frame.task)


def same_row(got, want) -> bool:
    """Equal, FLOAT columns within one f32 ulp (a re-associated fp64 sum may round the other way: tests/conftest.py)."""
    if list(got) != list(want):
        return False
    for k in got:
        g, w = got[k], want[k]
        if type(g) is not type(w) or (f32_ulps(f32(g), f32(w)) > 1 if type(g) is float else g != w):
            return False
    return True


def assert_ordered(got, unsorted, keys, limit=None):
    """`got` against the oracle's rows sorted in Python: the same key sequence, exactly; inside every run of equal keys
    the same rows as a multiset - with a LIMIT, every row of a run that the cut shortens is one of the run's, counted."""
    want = list(unsorted)
    for name, ascending in reversed(keys):
        want.sort(key=lambda r: r[name], reverse=not ascending)  # noqa: B023
    n = len(want) if limit is None else min(limit, len(want))
    key_of = lambda r: tuple(r[name] for name, _ in keys)  # noqa: E731
    assert [key_of(r) for r in got] == [key_of(r) for r in want[:n]]
    for key in dict.fromkeys(key_of(r) for r in got):
        mine = [r for r in got if key_of(r) == key]
        theirs = [r for r in want if key_of(r) == key]
        if limit is None:
            assert len(mine) == len(theirs)
        for r in mine:
            match = next((j for j, w in enumerate(theirs) if same_row(r, w)), None)
            assert match is not None, f"{r} is not a row of key {key}"
            del theirs[match]


def orders_select(api, paths):
    C = api.Col
    return (api.DataFrame().table(paths["orders"]).filter(C("price") > 26)
            .select(C("product"), C("quantity"), C("order_id"), C("price")))


def test_select_where_order_by_string_then_integer_desc(engine):
    from minispark_amd.workloads import engine_api

    g = load_golden("e2e_where_float_gt")
    api = engine_api(engine)
    unsorted = oracle_rows(orders_select(api, g["paths"]))
    keys = [("product", True), ("quantity", False)]  # quantity ties inside a product: runs of equal keys
    got = orders_select(api, g["paths"]).order_by(api.Col("product"), api.Col("quantity").desc()).collect()
    assert len(got) == len(unsorted) > 8
    assert_ordered(got, unsorted, keys)
    text = (f"SELECT product, quantity, order_id, price FROM '{g['paths']['orders']}' WHERE price > 26 "
            "ORDER BY product, quantity DESC;")
    assert_ordered(engine.sql(text).collect(), unsorted, keys)
    unique = [("product", False), ("order_id", True)]  # unique keys: the rows are pinned one by one
    got = orders_select(api, g["paths"]).order_by(api.Col("product").desc(), api.Col("order_id")).limit(4).collect()
    assert len(got) == 4
    assert_ordered(got, unsorted, unique, 4)


def many_groups_sorted(api, paths):
    return case_by_name("many_groups").build(api, paths).order_by(api.Col("max_price").desc(), api.Col("bucket")).limit(10)


MANY_KEYS = [("max_price", False), ("bucket", True)]  # MAX of stored f32 values is exact; bucket makes the key unique


@pytest.mark.parametrize("short_tail", ["1", "0"])
def test_group_by_order_by_float_aggregate_desc_limit(monkeypatch, short_tail):
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    monkeypatch.setenv("HIPSPARK_SHORT_TAIL", short_tail)
    g = load_golden("many_groups")
    with HipExecutionEngine() as e:
        assert e.short_tail_enabled == (short_tail == "1")
        api = engine_api(e)
        unsorted = oracle_rows(case_by_name("many_groups").build(api, g["paths"]))
        frame = many_groups_sorted(api, g["paths"])
        runs = [frame.collect() for _ in range(3)]  # the third run would be a recorded replay for an unsorted query
        assert len(runs[0]) == 10
        assert_ordered(runs[0], unsorted, MANY_KEYS, 10)
        assert runs[1] == runs[0] and runs[2] == runs[0]
        everything = case_by_name("many_groups").build(api, g["paths"]).order_by(api.Col("max_price").desc(), api.Col("bucket"))
        assert_ordered(everything.collect(), unsorted, MANY_KEYS)


def test_join_order_by_two_keys_limit(engine):
    from minispark_amd.workloads import engine_api

    g = load_golden("e2e_join_select")
    api = engine_api(engine)
    build = case_by_name("e2e_join_select").build
    unsorted = oracle_rows(build(api, g["paths"]))
    keys = [("first_name", False), ("product", True)]
    got = build(api, g["paths"]).order_by(api.Col("u.first_name").desc(), api.Col("o.product")).limit(5).collect()
    assert len(got) == 5 and list(got[0]) == ["first_name", "product"]
    assert_ordered(got, unsorted, keys, 5)
    text = (f"SELECT u.first_name, o.product FROM '{g['paths']['users']}' AS u JOIN '{g['paths']['orders']}' AS o "
            "ON u.user_id=o.user_id ORDER BY u.first_name DESC, o.product LIMIT 5;")
    assert_ordered(engine.sql(text).collect(), unsorted, keys, 5)


def test_group_by_having_order_by(engine):
    from minispark_amd.workloads import engine_api

    g = load_golden("e2e_group_sum_max")
    api = engine_api(engine)
    C, F = api.Col, api.F
    grouped = lambda: (api.DataFrame().table(g["paths"]["orders"]).group_by(C("product"))  # noqa: E731
                       .agg(F.count().alias("n"), F.max(C("price")).alias("top"), F.count().alias("_having_count"))
                       .filter(C("_having_count") > 3).select(C("product"), C("n"), C("top")))
    unsorted = oracle_rows(grouped())
    assert len(unsorted) >= 3
    keys = [("n", False), ("top", True)]  # n ties between products; top (a MAX: exact) breaks them
    assert_ordered(grouped().order_by(C("n").desc(), C("top")).collect(), unsorted, keys)
    text = (f"SELECT product, COUNT() AS n, MAX(price) AS top FROM '{g['paths']['orders']}' GROUP BY product "
            "HAVING COUNT() > 3 ORDER BY n DESC, top;")
    assert_ordered(engine.sql(text).collect(), unsorted, keys)


def test_limit_without_order_by_keeps_rows_of_the_unsorted_result(engine):
    from minispark_amd.workloads import engine_api

    g = load_golden("e2e_where_float_gt")
    api = engine_api(engine)
    unsorted = oracle_rows(orders_select(api, g["paths"]))
    for got in (orders_select(api, g["paths"]).limit(3).collect(),
                engine.sql(f"SELECT product, quantity, order_id, price FROM '{g['paths']['orders']}' WHERE price > 26 LIMIT 3;")
                .collect()):
        assert len(got) == 3
        left = list(unsorted)
        for r in got:
            match = next((j for j, w in enumerate(left) if same_row(r, w)), None)
            assert match is not None
            del left[match]
    assert orders_select(api, g["paths"]).limit(0).collect() == []
    assert len(orders_select(api, g["paths"]).limit(1000).collect()) == len(unsorted)


def test_a_repeated_query_returns_the_same_rows(engine):
    from minispark_amd.workloads import engine_api

    g = load_golden("q1_multiblock")
    api = engine_api(engine)
    C, F = api.Col, api.F
    frame = (api.DataFrame().table(g["paths"]["lineitem"]).group_by(C("l_shipmode"))
             .agg(F.count().alias("n"), F.max(C("l_extendedprice")).alias("top")).order_by(C("top").desc()).limit(5))
    unsorted = oracle_rows(api.DataFrame().table(g["paths"]["lineitem"]).group_by(C("l_shipmode"))
                           .agg(F.count().alias("n"), F.max(C("l_extendedprice")).alias("top")))
    runs = [frame.collect() for _ in range(3)]
    assert_ordered(runs[0], unsorted, [("top", False)], 5)
    assert runs[0] == runs[1] == runs[2]


def test_a_streamed_select_with_order_by_is_refused():
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from minispark_amd.workloads import engine_api

    g = load_golden("q1_multiblock")
    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: the table streams in several ranges (tests/test_gpu_streaming.py)
        api = engine_api(e)
        C, F = api.Col, api.F
        select = api.DataFrame().table(g["paths"]["lineitem"]).select(C("l_orderkey"), C("l_quantity"))
        with pytest.raises(ExecutionError, match=r"ORDER BY.*HIPSPARK_HBM_BUDGET"):
            select.order_by(C("l_quantity")).collect()
        # a streamed scan that feeds a GROUP BY is sorted as usual: the sort sits in the final stage
        grouped = (api.DataFrame().table(g["paths"]["lineitem"]).group_by(C("l_returnflag"))
                   .agg(F.max(C("l_extendedprice")).alias("top")))
        unsorted = oracle_rows(grouped)
        got = (api.DataFrame().table(g["paths"]["lineitem"]).group_by(C("l_returnflag"))
               .agg(F.max(C("l_extendedprice")).alias("top")).order_by(C("top")).collect())
        assert e.streamed_ranges >= 4
        assert_ordered(got, unsorted, [("top", True)])


def test_two_ranks_order_the_gathered_result_on_rank_0(tmp_path):
    from minispark_amd.workloads import api_namespace
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit

    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_order_by", "many_groups_sorted", "many_groups", out,
               "--runs", "3", "--hex-floats"])
    g = load_golden("many_groups")
    api = api_namespace(lambda: DataFrame(object()), Col, Functions, Lit)
    unsorted = oracle_rows(case_by_name("many_groups").build(api, g["paths"]))
    got = [{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in r.items()} for r in json.loads(out.read_text())]
    assert len(got) == 10
    assert_ordered(got, unsorted, MANY_KEYS, 10)
