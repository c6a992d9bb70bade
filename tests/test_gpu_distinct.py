"""SELECT DISTINCT on the GPU.  At the C ABI (hs_distinct) the surviving rows must be EXACTLY the first occurrences that
plain Python finds (dict.fromkeys over the row tuples, -0.0 as 0.0, every NaN as one token): nothing is computed, so
nothing is tolerated.  End to end: queries over the committed golden tables, through engine.sql and the DataFrame API,
against the rows of the same query without DISTINCT, deduplicated in Python."""

from __future__ import annotations

import ctypes as C
import json
import math
import re

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from tests.conftest import ROOT, load_golden
from tests.queries import case_by_name
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu


def _constants(*files):
    """The `constexpr int NAME = expression;` lines of the kernel sources, evaluated: the tile sizes come from the code."""
    env: dict[str, int] = {"HS_WAVE": 64}
    for name in files:
        for m in re.finditer(r"constexpr int (\w+) = ([^;]+);", (ROOT / "minispark_amd" / "csrc" / name).read_text()):
            try:
                env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))  # noqa: S307 - the repository's own source
            except Exception:  # noqa: BLE001, S112 - an expression over names this reader does not follow
                continue
    return env


_K = _constants("hs_ops.hip", "hs_radix.hip")
RX_TILE = _K["RX_TILE"]          # rows of one partition-pass workgroup of the sort
HEADS_TILE = _K["OB_TILE"]       # rows of one k_distinct_heads workgroup
COMPACT_TILE = _K["TILE_U8"]     # rows of one workgroup of hs_compact's byte-mask kernels
SIZES = [0, 1, 2, 63, 64, 65, RX_TILE - 1, RX_TILE, RX_TILE + 1, 3 * COMPACT_TILE + RX_TILE + 17]
NAN = object()


def test_the_tile_sizes_were_found_in_the_code():
    assert (RX_TILE, HEADS_TILE, COMPACT_TILE) == (8192, 2048, 4096)
    assert SIZES[-1] > 2 * COMPACT_TILE and SIZES[-1] > 2 * HEADS_TILE


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def token(v):
    if isinstance(v, float):
        return NAN if math.isnan(v) else (0.0 if v == 0.0 else v)
    return v


def first_rows(columns, n):
    """Plain Python: the first input index of every distinct row."""
    rows = [tuple(token(col[i]) for col in columns) for i in range(n)]
    first = dict.fromkeys(rows)      # the distinct rows, in the order of their first occurrence ...
    for i in reversed(range(n)):
        first[rows[i]] = i           # ... and where that was
    return list(first.values())


def upload(dev, values, col_type):
    from minispark_amd.io import StrCol

    if col_type == T.STRING:
        raw = [v if isinstance(v, bytes) else v.encode("utf-8") for v in values]
        data = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        return dev.upload_raw(StrCol(np.array([len(b) for b in raw], dtype=np.uint8), data), T.STRING)
    dtype = {T.INTEGER: np.int32, T.FLOAT: np.float32, T.TIMESTAMP: np.int64}[col_type]
    return dev.upload_raw(np.asarray(values, dtype=dtype), col_type)


def py_values(values, col_type):
    if col_type == T.FLOAT:
        return [float(v) for v in np.asarray(values, dtype=np.float32)]
    if col_type == T.STRING:
        return [v if isinstance(v, bytes) else v.encode("utf-8") for v in values]
    return [int(v) for v in values]


def hs_distinct(dev, cols, n, nrows_dev=None, n_keys=None):
    """The entry point itself -> (return code, surviving rows)."""
    import torch

    from minispark_amd import hipspark as hs

    lib = dev._raw_lib
    n_keys = len(cols) if n_keys is None else n_keys
    arr = (hs.hs_col * max(len(cols), 1))(*[c.as_hs() for c in cols])
    perm = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev.device)
    ws = torch.empty(int(lib.hs_distinct_ws_bytes(n, n_keys, 32 * max(n_keys, 1))) + 256, dtype=torch.uint8, device=dev.device)
    count = C.c_int64(-5)
    rc = lib.hs_distinct(dev.stream, arr, n_keys, n, nrows_dev, perm.data_ptr(), C.byref(count), ws.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, (perm[:count.value].cpu().tolist() if rc == 0 else None)


def check(dev, columns):
    """columns = [(values, ColumnType)]: hs_distinct over all of them against Python's first occurrences, exactly."""
    n = len(columns[0][0])
    cols = [upload(dev, v, t) for v, t in columns] if n else []
    want = first_rows([py_values(v, t) for v, t in columns], n)
    if n == 0:  # no buffer to point at: the call answers before it looks at the columns
        cols = [upload(dev, [0], T.INTEGER)]
    rc, got = hs_distinct(dev, cols, n)
    assert rc == 0 and got == want
    return got


@pytest.mark.parametrize("n", SIZES)
def test_i32_rows_at_every_tile_boundary(dev, n):
    rng = np.random.default_rng(n + 1)
    check(dev, [(rng.integers(-2**31, 2**31, n, dtype=np.int64), T.INTEGER)])   # (almost) all rows distinct
    check(dev, [(np.arange(n) * 7 - 3, T.INTEGER)])                           # all rows distinct
    check(dev, [(rng.integers(-3, 4, n), T.INTEGER)])                         # 7 values
    got = check(dev, [(np.full(n, -77), T.INTEGER)])                          # all rows equal: every pass is skipped
    assert got == ([0] if n else [])
    if n >= 2:
        v = np.arange(n) + 10
        v[-1] = v[0]                                                          # one duplicate pair: first and last row
        assert check(dev, [(v, T.INTEGER)]) == list(range(n - 1))


def test_a_duplicate_pair_across_a_tile_boundary_of_the_heads_kernel(dev):
    n = 2 * HEADS_TILE + 5
    for edge in (HEADS_TILE, 2 * HEADS_TILE, 64, HEADS_TILE + 64):  # sorted positions edge - 1 and edge hold equal rows
        v = np.arange(n) * 2                # sorted already: sorted position = row
        v[edge] = v[edge - 1]
        assert check(dev, [(v, T.INTEGER)]) == [i for i in range(n) if i != edge]
        rng = np.random.default_rng(edge)
        shuffle = rng.permutation(n)        # ... and with the rows in any order: the earlier of the two rows survives
        got = check(dev, [(v[shuffle], T.INTEGER)])
        pair = sorted(int(j) for j in np.nonzero(v[shuffle] == v[edge])[0])
        assert len(pair) == 2 and pair[0] in got and pair[1] not in got


def test_a_one_word_key_gives_the_same_rows_with_the_words_formed_again(dev, monkeypatch):
    rng = np.random.default_rng(2)
    n = RX_TILE + HEADS_TILE + 3
    monkeypatch.setenv("HIPSPARK_DISTINCT_GATHER", "1")  # read at every call: the path of longer keys on a one-word key
    check(dev, [(rng.integers(-40, 40, n), T.INTEGER)])
    check(dev, [(rng.integers(-4, 4, n), T.INTEGER), (rng.integers(0, 9, n), T.INTEGER)])


def test_two_i32_columns_share_one_word(dev):
    rng = np.random.default_rng(3)
    n = RX_TILE + 77
    a, b = rng.integers(-4, 4, n), rng.integers(-2**31, -2**31 + 6, n)
    got = check(dev, [(a, T.INTEGER), (b, T.INTEGER)])
    assert 8 < len(got) <= 48
    check(dev, [(b, T.INTEGER), (a, T.INTEGER)])
    check(dev, [(a, T.INTEGER), (a, T.INTEGER)])


def test_three_word_keys_that_differ_in_one_word_only(dev):
    rng = np.random.default_rng(4)
    n = HEADS_TILE + 130
    big = np.full(n, (0x1234 << 48) + 99, dtype=np.int64)
    few = rng.integers(-3, 3, n)
    got = check(dev, [(big, T.TIMESTAMP), (big, T.TIMESTAMP), (few, T.INTEGER)])  # I64 + I64 + I32: the last word differs
    assert len(got) == 6
    first = (rng.integers(-3, 3, n).astype(np.int64) << 40) - 1
    got = check(dev, [(first, T.TIMESTAMP), (big, T.TIMESTAMP), (np.full(n, 8), T.INTEGER)])  # the first word differs
    assert len(got) == 6
    check(dev, [(first, T.TIMESTAMP), (big, T.TIMESTAMP), (few, T.INTEGER)])


def test_f32_rows_compare_like_the_sort_and_the_first_occurrence_keeps_its_bits(dev):
    bits = np.array([0x80000000, 0x00000000, 0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x80000001,
                     0x00000001, 0x7f800001, 0x3f800000, 0x00000000, 0x7f800000, 0x80000001, 0x007fffff], dtype=np.uint32)
    values = bits.view(np.float32)  # -0.0 first, then +0.0; NaNs of several payloads and signs; +-inf; denormals
    got = check(dev, [(values, T.FLOAT)])
    assert got == [0, 2, 4, 5, 6, 7, 10, 14]
    assert bits[got[0]] == 0x80000000 and bits[got[1]] == 0x7fc00000  # the survivors are the FIRST rows: -0.0, the first NaN
    rng = np.random.default_rng(5)
    n = RX_TILE + 9
    many = rng.choice(values, n)
    tie = rng.integers(0, 2, n)
    got = check(dev, [(many, T.FLOAT), (tie, T.INTEGER)])
    assert len(got) == 16
    col = upload(dev, many, T.FLOAT)  # through Device.distinct + gather: the bits that come back are the survivors' own
    from minispark_amd.device import DBatch

    batch = DBatch([("f", T.FLOAT)], [col], n)
    perm, count = dev.distinct(batch)
    kept = dev.download(dev.gather_batch(batch, perm, count).cols[0], T.FLOAT).view(np.uint32)
    assert kept.tolist() == many.view(np.uint32)[first_rows([py_values(many, T.FLOAT)], n)].tolist()


def test_string_rows_compare_by_bytes_and_length(dev):
    pool = [b"", b"a", b"a\0", b"ab", b"a\0\0", b"x" * 254 + b"y", b"x" * 254 + b"z", b"x" * 255, b"abcdefgh", b"abcdefghi",
            "é".encode(), b"b"]
    assert check(dev, [(pool, T.STRING)]) == list(range(len(pool)))   # all different: '' / 'a' / 'a\0' / 'ab' / 255 bytes
    rng = np.random.default_rng(6)
    n = HEADS_TILE + 200
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    assert len(check(dev, [(words, T.STRING)])) == len(pool)
    check(dev, [(words, T.STRING), (rng.integers(0, 3, n), T.INTEGER)])
    assert check(dev, [([b""] * 70, T.STRING)]) == [0]                  # only empty strings: a key of one length byte
    fixed = [b"%04d-ab" % (j % 11) for j in rng.integers(0, 1000, n)]   # one length: a fixed-length column, no length byte
    col = upload(dev, fixed, T.STRING)
    assert col.as_hs().fixed_len == 7
    assert len(check(dev, [(fixed, T.STRING)])) == 11


def test_a_dictionary_coded_column_with_an_integer(dev):
    rng = np.random.default_rng(7)
    n = 5000
    pool = ["", "a", "ab", "b", "kiwi", "x" * 40]
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    nums = rng.integers(0, 4, n)
    coded = dev.dict_encode(upload(dev, words, T.STRING))
    assert coded is not None and coded.dict is not None
    rc, got = hs_distinct(dev, [coded, upload(dev, nums, T.INTEGER)], n)
    assert rc == 0 and got == first_rows([py_values(words, T.STRING), py_values(nums, T.INTEGER)], n) and len(got) == 24


def test_a_lazy_batch_is_deduplicated_up_to_its_device_row_count(dev):
    import torch

    from minispark_amd.device import DBatch

    n = RX_TILE + 500
    rows = n - 300  # what the device says; the buffers hold n rows
    values = np.arange(n) % 1000
    values[rows:] = 5000 + np.arange(n - rows)  # rows past the count would all survive
    col = upload(dev, values, T.INTEGER)
    count_dev = torch.tensor([rows], dtype=torch.int64, device=dev.device)
    rc, got = hs_distinct(dev, [col], n, count_dev.data_ptr())
    assert rc == 0 and got == list(range(1000))
    perm, count = dev.distinct(DBatch([("c0", T.INTEGER)], [col], n, None, count_dev))
    assert count == 1000 and perm.cpu().tolist() == list(range(1000))


def test_thirteen_keys_are_an_error_code_not_a_launch(dev):
    col = upload(dev, [1, 2, 3], T.INTEGER)
    rc, _ = hs_distinct(dev, [col] * 13, 3)
    assert rc == 2 and b"12" in dev._raw_lib.hs_last_error()
    rc, got = hs_distinct(dev, [col] * 12, 3)
    assert rc == 0 and got == [0, 1, 2]


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine() as e:
        yield e


@pytest.fixture(scope="module")
def api(engine):
    from minispark_amd.workloads import engine_api

    return engine_api(engine)


def oracle_rows(frame):
    from oracle.py_engine import run_query

    return run_query(frame.task)


def tuples(rows):
    return [tuple(r.values()) for r in rows]


def assert_deduplicated(got, plain, oracle, in_order=True):
    """`got` = DISTINCT of the engine's own undeduplicated rows `plain`, exactly and (where the engine returns rows in a
    fixed order: scans and joins, not hash-grouped rows) in their order; as a set it is the oracle's.  Only columns
    whose values are exact (strings, integers, counts, MAX of stored floats) are compared this way."""
    want = list(dict.fromkeys(tuples(plain)))
    assert tuples(got) == want if in_order else sorted(tuples(got)) == sorted(want)
    assert set(tuples(got)) == set(tuples(oracle)) and len(got) == len(set(tuples(oracle)))


LINEITEM = lambda: load_golden("q1_multiblock")["paths"]["lineitem"]  # noqa: E731 - 6000 rows, 7 ship modes, several blocks


def test_one_string_column_with_few_values(engine, api):
    frame = lambda: api.DataFrame().table(LINEITEM()).select(api.Col("l_shipmode"))  # noqa: E731
    oracle = oracle_rows(frame())
    got = engine.sql(f"SELECT DISTINCT l_shipmode FROM '{LINEITEM()}';").collect()
    assert len(got) == 7 < len(oracle)
    assert_deduplicated(got, frame().collect(), oracle)
    assert frame().distinct().collect() == got


def test_a_string_and_an_integer_column(engine, api):
    frame = lambda: api.DataFrame().table(LINEITEM()).select(api.Col("l_shipmode"), api.Col("l_orderkey"))  # noqa: E731
    oracle = oracle_rows(frame())
    got = engine.sql(f"SELECT DISTINCT l_shipmode, l_orderkey FROM '{LINEITEM()}';").collect()
    assert 7 < len(got) < len(oracle)
    assert_deduplicated(got, frame().collect(), oracle)


def country_product(api, paths):
    C = api.Col
    return (api.DataFrame().table(paths["users"]).alias("u")
            .join(api.DataFrame().table(paths["orders"]).alias("o"), on=C("u.user_id") == C("o.user_id"), how="inner")
            .select(C("u.country"), C("o.product")))


def test_distinct_over_the_rows_of_a_join(engine, api):
    g = load_golden("e2e_join_select")
    oracle = oracle_rows(country_product(api, g["paths"]))
    got = country_product(api, g["paths"]).distinct().collect()
    assert list(got[0]) == ["country", "product"] and len(got) < len(oracle)
    assert_deduplicated(got, country_product(api, g["paths"]).collect(), oracle)
    text = (f"SELECT DISTINCT u.country, o.product FROM '{g['paths']['users']}' AS u JOIN '{g['paths']['orders']}' AS o "
            "ON u.user_id=o.user_id;")
    assert engine.sql(text).collect() == got


def test_distinct_then_order_by_desc_and_limit(engine, api):
    frame = lambda: api.DataFrame().table(LINEITEM()).select(api.Col("l_shipmode"), api.Col("l_orderkey"))  # noqa: E731
    want = sorted(sorted(set(tuples(oracle_rows(frame()))), key=lambda r: r[1], reverse=True), key=lambda r: r[0], reverse=True)
    got = frame().distinct().order_by(api.Col("l_shipmode").desc(), api.Col("l_orderkey").desc()).limit(9).collect()
    assert tuples(got) == want[:9]  # every column is a key and the rows are distinct: the order is total
    text = f"SELECT DISTINCT l_shipmode, l_orderkey FROM '{LINEITEM()}' ORDER BY l_shipmode DESC, l_orderkey DESC LIMIT 9;"
    assert engine.sql(text).collect() == got
    everything = frame().distinct().order_by(api.Col("l_shipmode").desc(), api.Col("l_orderkey").desc()).collect()
    assert tuples(everything) == want
    head = frame().distinct().limit(5).collect()  # LIMIT without keys: the head of the survivors
    assert head == frame().distinct().collect()[:5] and len(head) == 5


def test_distinct_on_a_group_by_result(engine, api):
    C, F = api.Col, api.F
    grouped = lambda: (api.DataFrame().table(LINEITEM()).group_by(C("l_shipmode"))  # noqa: E731
                       .agg(F.count().alias("n"), F.max(C("l_extendedprice")).alias("top")).select(C("l_shipmode"), C("n"), C("top")))
    oracle = oracle_rows(grouped())
    got = grouped().distinct().collect()
    assert len(got) == len(oracle) == 7  # the key column makes every row different: nothing goes
    assert_deduplicated(got, grouped().collect(), oracle, in_order=False)
    # without the key column the rows do collapse: 1500 orders, every one of them with the same number of lines
    counts = lambda: (api.DataFrame().table(LINEITEM()).group_by(C("l_orderkey")).agg(F.count().alias("n"))  # noqa: E731
                      .select(C("n")))
    oracle = oracle_rows(counts())
    got = counts().distinct().collect()
    assert len(got) == len(set(tuples(oracle))) < len(oracle)
    assert_deduplicated(got, counts().collect(), oracle, in_order=False)
    many = load_golden("many_groups")
    per_bucket = lambda: case_by_name("many_groups").build(api, many["paths"]).select(C("count"))  # noqa: E731
    oracle = oracle_rows(per_bucket())
    got = per_bucket().distinct().collect()
    assert 1 < len(got) == len(set(tuples(oracle))) < len(oracle)
    assert set(tuples(got)) == set(tuples(oracle))


def test_a_repeated_query_returns_the_same_rows(engine, api):
    frame = api.DataFrame().table(LINEITEM()).select(api.Col("l_returnflag"), api.Col("l_shipmode")).distinct()
    runs = [frame.collect() for _ in range(3)]  # the third run would be a recorded replay without the SortTask
    assert runs[0] == runs[1] == runs[2] and len(runs[0]) == len(set(tuples(runs[0]))) > 7


def test_a_streamed_select_with_distinct_is_refused():
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from minispark_amd.workloads import engine_api

    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: the table streams in several ranges (tests/test_gpu_streaming.py)
        api = engine_api(e)
        select = api.DataFrame().table(LINEITEM()).select(api.Col("l_orderkey"), api.Col("l_shipmode"))
        with pytest.raises(ExecutionError, match=r"DISTINCT.*HIPSPARK_HBM_BUDGET"):
            select.distinct().collect()


def test_more_columns_than_the_kernel_compares_is_an_execution_error(engine, api):
    from minispark_amd.execution import ExecutionError

    wide = lambda k: api.DataFrame().table(LINEITEM()).select(  # noqa: E731
        api.Col("l_shipmode"), *[api.Col("l_orderkey").alias(f"k{j}") for j in range(k - 1)])
    with pytest.raises(ExecutionError, match=r"DISTINCT.*12"):
        wide(13).distinct().collect()
    got = wide(12).distinct().collect()
    assert len(got[0]) == 12 and len(got) == len(set(tuples(got))) == 4883


def two_rank_frame(api, paths):
    return (api.DataFrame().table(paths["lineitem"]).select(api.Col("l_shipmode"), api.Col("l_returnflag")).distinct()
            .order_by(api.Col("l_shipmode"), api.Col("l_returnflag").desc()))


def test_two_ranks_deduplicate_the_gathered_result_on_rank_0(tmp_path):
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    out = tmp_path / "rows.json"
    run_ranks([ROOT / "tests" / "result_rows_worker.py", "tests.test_gpu_distinct", "two_rank_frame", "q1_multiblock", out])
    api = api_namespace(lambda: DataFrame(object()), Col, Functions, Lit)
    paths = load_golden("q1_multiblock")["paths"]
    plain = api.DataFrame().table(paths["lineitem"]).select(api.Col("l_shipmode"), api.Col("l_returnflag"))
    want = sorted(sorted(set(tuples(oracle_rows(plain))), key=lambda r: r[1], reverse=True), key=lambda r: r[0])
    got = [tuple(r) for r in json.loads(out.read_text())]
    assert got == want and len(got) > 7
