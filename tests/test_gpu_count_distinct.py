"""COUNT(DISTINCT e) on the GPU.  At the C ABI (hs_mark_first) the marks must be EXACTLY those of the Python model
(tests/count_distinct_model.py), on the sort path, on the dense path where it applies, and in mode 0.  End to end the counts
are those of plain Python over the tables' rows, and every other aggregate of the same query equals, bit for bit, what the
CPU oracle returns for the query without the distinct item.  Marks and counts are integers: nothing is tolerated."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from minispark_amd.constants import ColumnType as T
from oracle.compare import assert_rows_match
from tests.conftest import ROOT, load_golden
from tests.count_distinct_model import counts, marks
from tests.ranks import run_ranks
from tests.test_gpu_distinct import _constants, py_values, upload

pytestmark = pytest.mark.gpu

_K = _constants("hs_ops.hip", "hs_radix.hip")
RX_TILE = _K["RX_TILE"]          # rows of one partition-pass workgroup of the sort
OB_TILE = _K["OB_TILE"]          # rows of one k_distinct_heads workgroup
DENSE_BITS = _K["MF_DENSE_BITS"]  # varying bits the dense path holds
SIZES = [1, 2, 63, 64, 65, OB_TILE - 1, OB_TILE, OB_TILE + 1, RX_TILE - 1, RX_TILE, RX_TILE + 1, 3 * RX_TILE + 17]
CANARY = 0x5A5A5A5A
OK, E_LIMIT = 0, 2


def test_the_constants_were_found_in_the_code():
    assert (RX_TILE, OB_TILE) == (8192, 2048) and 1 <= DENSE_BITS <= 28


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def hs_mark_first(dev, cols, n, sel=None, mode=0):
    """The entry point itself, over a mark buffer longer than the rows -> (return code, marks); the cells past the rows
    must keep their canary."""
    import torch

    from minispark_amd import hipspark as hs

    lib = dev._raw_lib
    arr = (hs.hs_col * len(cols))(*[c.as_hs() for c in cols])
    out = torch.full((n + 64,), CANARY, dtype=torch.int32, device=dev.device)
    ws = torch.empty(int(lib.hs_mark_first_ws_bytes(n, len(cols), 32 * len(cols))) + 256, dtype=torch.uint8, device=dev.device)
    sel_dev = None if sel is None else torch.tensor(list(sel) or [0], dtype=torch.int64, device=dev.device)
    rc = lib.hs_mark_first(dev.stream, arr, len(cols), n, None if sel is None else sel_dev.data_ptr(),
                           0 if sel is None else len(sel), mode, out.data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    host = out.cpu().tolist()
    assert host[n:] == [CANARY] * 64, "cells past the rows were written"
    return rc, host[:n]


def sel_lists(n):
    """None, every row, every third row, one row, no row, and the second half (first occurrences lie outside it)."""
    return [None, list(range(n)), list(range(0, n, 3)), [n // 2], [], list(range(n // 2, n))]


def key_words(columns, codes=None):
    """The rows' sort keys as hs_order_by lays them out (include/hipspark.h): per column a run of bytes - INTEGER and
    TIMESTAMP big-endian with the sign bit flipped, FLOAT with the sign-dependent flip (-0.0 as +0.0, every NaN one value),
    a STRING of one length as its bytes, of several lengths zero-padded to the column's longest and followed by the length
    byte, a dictionary-coded column (``codes``: {column index: its code bytes}) as the code - concatenated.  -> one integer
    per row, the key's bytes left-aligned in 64 bits, or None when the key is longer than one word."""
    n = len(columns[0][0])
    runs = []
    for c, (values, col_type) in enumerate(columns):
        if codes and c in codes:
            runs.append([bytes([int(v)]) for v in codes[c]])
        elif col_type == T.STRING:
            raw = [v if isinstance(v, bytes) else v.encode("utf-8") for v in values]
            longest = max(map(len, raw))
            fixed = all(len(b) == longest for b in raw)
            runs.append([b if fixed else b.ljust(longest, b"\0") + bytes([len(b)]) for b in raw])
        elif col_type == T.FLOAT:
            bits = np.asarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)
            bits = np.where((bits & 0x7fffffff) > 0x7f800000, 0x7fc00000, bits)
            bits = np.where(bits == 0x80000000, 0, bits)
            bits = np.where(bits & 0x80000000, ~bits & 0xffffffff, bits | 0x80000000)
            runs.append([int(b).to_bytes(4, "big") for b in bits])
        else:
            size = 4 if col_type == T.INTEGER else 8
            runs.append([(int(v) + (1 << (8 * size - 1))).to_bytes(size, "big") for v in values])
    if sum(len(run[0]) for run in runs) > 8:
        return None
    return [int.from_bytes(b"".join(run[r] for run in runs).ljust(8, b"\0"), "big") for r in range(n)]


def dense_fits(words, considered):
    """Whether the dense path holds this key over the considered rows: one word, at most DENSE_BITS varying bits in at most
    8 contiguous runs."""
    if words is None:
        return False
    both, either = ~0, 0
    for r in considered:
        both, either = both & words[r], either | words[r]
    v = (both ^ either) & (2**64 - 1)
    runs = sum(1 for b in range(64) if (v >> b) & 1 and not (b and (v >> (b - 1)) & 1))
    return bin(v).count("1") <= DENSE_BITS and runs <= 8


def check(dev, columns, dense, sels=None, cols=None, codes=None):
    """columns = [(values, ColumnType)]: hs_mark_first over all of them as keys against the model, exactly, for every row
    list, on the sort path (mode 1), in mode 0 and on the dense path (mode 2), whose return code must be exactly what the
    key words of the CONSIDERED rows say: HS_OK where they fit, HS_E_LIMIT where they do not.  ``dense`` states what the
    case is about: whether the path applies over all rows."""
    n = len(columns[0][0])
    cols = cols or [upload(dev, v, t) for v, t in columns]
    values = [py_values(v, t) for v, t in columns]
    words = key_words(columns, codes)
    assert dense_fits(words, range(n)) == dense, "the case is not the one it says"
    for sel in sel_lists(n) if sels is None else sels:
        want = marks(values, sel)
        rc, got = hs_mark_first(dev, cols, n, sel, mode=1)
        assert rc == OK and got == want, ("sort path", n, None if sel is None else len(sel))
        rc, got = hs_mark_first(dev, cols, n, sel, mode=0)
        assert rc == OK and got == want, ("mode 0", n, None if sel is None else len(sel))
        if sel is not None and len(sel) == 0:
            continue  # no row to look at: the call answers before it knows the key's bits
        rc, got = hs_mark_first(dev, cols, n, sel, mode=2)
        # (fewer considered rows, fewer varying bits: a key the dense path refuses over all rows may fit over some)
        if dense_fits(words, range(n) if sel is None else sel):
            assert rc == OK and got == want, ("dense path", n, None if sel is None else len(sel))
        else:
            assert rc == E_LIMIT and b"dense path" in dev._raw_lib.hs_last_error(), (n, None if sel is None else len(sel))


def i32_with_top_bytes(n, seed, negatives=True):
    """Small values and values that differ in the top byte only (7 varying bits in 3 runs); with negatives among them
    every bit of the key word varies."""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 16, n) + (rng.integers(0, 3, n) << 24) + (rng.integers(0, 2, n) << 30)
    return np.where(rng.integers(0, 3, n) == 0, -values - 1, values) if negatives else values


def _dense_applies(values):
    """Whether a ONE-column integer key of these values (all of them considered) has at most DENSE_BITS varying bits in at
    most 8 runs: the flip of the sign bit does not change which bits vary."""
    arr = np.asarray(values, dtype=np.int64).view(np.uint64)
    v = int(np.bitwise_and.reduce(arr) ^ np.bitwise_or.reduce(arr))
    runs = sum(1 for b in range(64) if (v >> b) & 1 and not (b and (v >> (b - 1)) & 1))
    return bin(v).count("1") <= DENSE_BITS and runs <= 8


@pytest.mark.parametrize("n", SIZES)
def test_one_i32_key_at_every_tile_boundary(dev, n):
    signed = i32_with_top_bytes(n, n)
    check(dev, [(signed, T.INTEGER)], dense=_dense_applies(signed.astype(np.int32)))
    assert n < 64 or not _dense_applies(signed.astype(np.int32))  # with negatives every bit varies: the sort path's case
    check(dev, [(i32_with_top_bytes(n, n, negatives=False), T.INTEGER)], dense=True)
    if n >= 2:
        v = np.arange(n) + 10
        v[-1] = v[0]  # all different but the first and the last row
        check(dev, [(v, T.INTEGER)], dense=True, sels=[None, list(range(1, n))])


def test_a_code_byte_and_an_integer_share_one_word(dev):
    rng = np.random.default_rng(1)
    n = RX_TILE + OB_TILE + 3
    pool = ["", "a", "ab", "b", "kiwi", "x" * 40]
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    nums = rng.integers(0, 40, n)
    coded = dev.dict_encode(upload(dev, words, T.STRING))
    assert coded is not None and coded.dict is not None
    cols = [coded, upload(dev, nums, T.INTEGER)]
    check(dev, [(words, T.STRING), (nums, T.INTEGER)], dense=True, cols=cols, codes={0: coded.data[:n].cpu().tolist()})


def test_i64_timestamps(dev):
    rng = np.random.default_rng(2)
    n = OB_TILE + 77
    near = 1_700_000_000_000_000 + rng.integers(0, 50, n) * 86_400_000_000  # 50 days: bits spread over the low word
    check(dev, [(near, T.TIMESTAMP)], dense=_dense_applies(near))
    far = np.where(rng.integers(0, 2, n) == 0, -(1 << 62), (1 << 62) + 5) + rng.integers(0, 3, n)
    check(dev, [(far, T.TIMESTAMP)], dense=_dense_applies(far))


def test_f32_zeros_nans_and_infinities(dev):
    bits = np.array([0x80000000, 0x00000000, 0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x80000001,
                     0x00000001, 0x7f800001, 0x3f800000, 0x00000000, 0x7f800000, 0x80000001, 0x007fffff], dtype=np.uint32)
    values = bits.view(np.float32)  # -0.0 then +0.0; NaNs of two payloads and both signs; +-inf; denormals
    rc, got = hs_mark_first(dev, [upload(dev, values, T.FLOAT)], len(values), None, mode=1)
    assert rc == OK and got == [1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 1]
    rng = np.random.default_rng(3)
    many = rng.choice(values, RX_TILE + 9)
    check(dev, [(many, T.FLOAT)], dense=False)  # the key words of these values vary in nearly every bit
    check(dev, [(rng.integers(0, 2, len(many)), T.INTEGER), (many, T.FLOAT)], dense=False)


def test_strings_compare_by_bytes_and_length(dev):
    pool = [b"", b"a", b"a\0", b"ab", b"a\0\0", b"x" * 254 + b"y", b"x" * 255, b"abcdefgh", b"abcdefghi", "é".encode()]
    rng = np.random.default_rng(4)
    n = OB_TILE + 200
    words = [pool[j] for j in rng.integers(0, len(pool), n)]
    check(dev, [(words, T.STRING)], dense=False)  # 256 bytes: 32 words
    rc, got = hs_mark_first(dev, [upload(dev, pool + pool, T.STRING)], 2 * len(pool), None, mode=0)
    assert rc == OK and got == [1] * len(pool) + [0] * len(pool)  # 'a', 'a\0' and '' are three values
    short = [pool[j] for j in rng.integers(0, 5, n)]  # up to 3 bytes + the length byte: one word
    check(dev, [(short, T.STRING)], dense=True, sels=[None, list(range(0, n, 3))])
    # a list whose rows hold shorter strings than the column's longest: the same marks
    longest_outside = [b"zz-the-longest"] + [pool[j] for j in rng.integers(0, 4, 99)]
    check(dev, [(longest_outside, T.STRING)], dense=False, sels=[list(range(1, 100))])


def test_two_word_and_three_word_keys(dev):
    rng = np.random.default_rng(5)
    n = RX_TILE + 130
    big = (rng.integers(0, 4, n).astype(np.int64) << 40) - 1
    few = rng.integers(-3, 3, n)
    check(dev, [(big, T.TIMESTAMP), (few, T.INTEGER)], dense=False)                       # 12 bytes: two words
    check(dev, [(few, T.INTEGER), (big, T.TIMESTAMP), (big, T.TIMESTAMP)], dense=False,   # 20 bytes: three words
          sels=[None, list(range(0, n, 3)), list(range(n // 2, n))])
    check(dev, [(np.full(n, 7), T.TIMESTAMP), (np.full(n, 8), T.TIMESTAMP)], dense=False, sels=[None, [5, 9]])  # nothing varies


def test_a_fixed_width_string_key_of_no_byte(dev):
    n = 70
    empty = upload(dev, [b""] * n, T.STRING)
    for sel, want in ((None, [1] + [0] * (n - 1)), ([3, 9], [0, 0, 0, 1] + [0] * (n - 4))):
        rc, got = hs_mark_first(dev, [empty], n, sel, mode=0)
        assert rc == OK and got == want


# ---- the dense path's edges ---------------------------------------------------------------------------------------------
def test_one_value_and_one_varying_bit(dev):
    n = OB_TILE + 5
    check(dev, [(np.full(n, -77), T.INTEGER)], dense=True)                     # popcount(V) = 0: a table of one slot
    rng = np.random.default_rng(6)
    check(dev, [(4 + rng.integers(0, 2, n), T.INTEGER)], dense=True)           # V = 1 bit
    check(dev, [(np.where(rng.integers(0, 2, n) == 0, -5, 2**31 - 5), T.INTEGER)], dense=True,
          sels=[None, list(range(0, n, 3))])                                   # V = the sign bit alone


def test_nine_separated_bits_are_more_runs_than_the_dense_path_takes(dev):
    rng = np.random.default_rng(7)
    n = OB_TILE + 9
    spread = sum(1 << (2 * j) for j in range(9))  # bits 0, 2, ..., 16
    values = np.where(rng.integers(0, 2, n) == 0, 0, spread) ^ (rng.integers(0, 2, n) << 4)
    values[:2] = [0, spread]
    assert not _dense_applies(values)
    check(dev, [(values, T.INTEGER)], dense=False, sels=[None, list(range(0, n, 3)), list(range(n // 2, n))])
    eight = values & ~(1 << 16)
    eight[:2] = [0, spread & ~(1 << 16)]
    check(dev, [(eight, T.INTEGER)], dense=True, sels=[None, list(range(0, n, 3))])  # 8 runs: the last that fit


@pytest.mark.parametrize("layout", ["one run", "eight runs"])
def test_exactly_dense_bits_and_one_more(dev, layout):
    rng = np.random.default_rng(8)
    n = 2 * RX_TILE  # sizes at which the choice of the path can go wrong, not workload sizes

    def spread(x, bits):
        if layout == "one run":
            return x
        per = bits // 8  # 8 runs of `per` bits, one zero bit between them; what is left joins the last run
        out = np.zeros_like(x)
        for r in range(8):
            take = per if r < 7 else bits - 7 * per
            out |= ((x >> (r * per)) & ((1 << take) - 1)) << (r * (per + 1))
        return out

    for bits, dense in ((DENSE_BITS, True), (DENSE_BITS + 1, False)):
        x = rng.integers(0, 1 << bits, n)
        x[:2] = [0, (1 << bits) - 1]       # every bit varies
        x[n // 2:] = x[: n - n // 2]       # ... and every value of the first half comes again
        values = spread(x, bits)
        assert _dense_applies(values) == dense
        check(dev, [(values, T.TIMESTAMP)], dense=dense, sels=[None, list(range(1, n, 2))])  # (8 runs of 25 bits: 33 bits)


def test_thirteen_keys_are_an_error_code_not_a_launch(dev):
    col = upload(dev, [1, 2, 1], T.INTEGER)
    rc, _ = hs_mark_first(dev, [col] * 13, 3)
    assert rc == E_LIMIT and b"12" in dev._raw_lib.hs_last_error()
    rc, got = hs_mark_first(dev, [col] * 12, 3, None, mode=1)
    assert rc == OK and got == [1, 1, 0]


def test_the_shared_sort_still_orders_and_deduplicates_the_same_inputs(dev):
    from tests.test_gpu_distinct import check as check_distinct
    from tests.test_gpu_order_by import check as check_order

    rng = np.random.default_rng(9)
    for n in (65, OB_TILE + 1, RX_TILE + 1):
        ints = i32_with_top_bytes(n, n)
        big = (rng.integers(0, 4, n).astype(np.int64) << 40) - 1
        check_distinct(dev, [(ints, T.INTEGER)])
        check_distinct(dev, [(big, T.TIMESTAMP), (ints, T.INTEGER)])
        check_order(dev, [(ints, T.INTEGER)], [True])
        check_order(dev, [(big, T.TIMESTAMP), (ints, T.INTEGER)], [False, True])
        check_order(dev, [(ints, T.INTEGER)], [True], limit=7)


def test_device_mark_first_returns_an_integer_column_and_poisons_the_recording(dev):
    from minispark_amd import hipspark as hs
    from minispark_amd.device import DBatch, DeviceError

    n = 1000
    rng = np.random.default_rng(10)
    a, b = rng.integers(0, 5, n), rng.integers(0, 7, n)
    batch = DBatch([("a", T.INTEGER), ("b", T.INTEGER)], [upload(dev, a, T.INTEGER), upload(dev, b, T.INTEGER)], n)
    rec = dev.start_recording()
    try:
        col = dev.mark_first(batch, [0, 1])
    finally:
        dev.stop_recording()
    assert rec.poisoned
    assert (col.kind, col.n) == (hs.I32, n)
    assert dev.download(col, T.INTEGER).tolist() == marks([py_values(a, T.INTEGER), py_values(b, T.INTEGER)])
    import torch

    sel = torch.arange(1, n, 2, dtype=torch.int64, device=dev.device)
    got = dev.download(dev.mark_first(batch, [1], sel, sel.numel()), T.INTEGER).tolist()
    assert got == marks([py_values(b, T.INTEGER)], list(range(1, n, 2)))
    with pytest.raises(DeviceError, match="1 to 12"):
        dev.mark_first(batch, [])


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


def table_rows(path):
    from minispark_amd.io import BlockFile

    return list(BlockFile(path).read_data_rows())


def key_of(row, keys):
    return None if not keys else row[keys[0]] if len(keys) == 1 else tuple(row[k] for k in keys)


def expected(rows, keys, value, alive=lambda r: True):
    """{group key: COUNT(DISTINCT value)} over the living rows, in plain Python; ``value`` = a column name or a function."""
    fn = value if callable(value) else (lambda r: r[value])
    return counts([key_of(r, keys) for r in rows], [fn(r) for r in rows], [alive(r) for r in rows])


def assert_counts_and_rest(got, keys, names, want_counts, oracle):
    """``got`` = result rows holding the key columns, the distinct counts ``names`` and other aggregates: every count is
    Python's, and the rows without the counts are the oracle's rows of the query without them, bit for bit."""
    assert len(got) == len(want_counts[0])
    for row in got:
        for name, want in zip(names, want_counts):
            assert type(row[name]) is int and row[name] == want[key_of(row, keys)], (name, key_of(row, keys))
    assert_rows_match([{k: v for k, v in row.items() if k not in names} for row in got], oracle)


LINEITEMS = ["q1_multiblock", "q1_ragged_blocks"]


@pytest.mark.parametrize("table", LINEITEMS)
def test_the_golden_tables_make_the_queries_bite(table):
    from minispark_amd.io import BlockFile

    path = load_golden(table)["paths"]["lineitem"]
    rows = table_rows(path)
    sizes = BlockFile(path).block_rows()
    assert len(sizes) == {"q1_multiblock": 6, "q1_ragged_blocks": 8}[table] and sum(sizes) == len(rows)
    block_of = [b for b, size in enumerate(sizes) for _ in range(size)]
    seen: dict = {}
    for r, row in enumerate(rows):
        seen.setdefault((row["l_returnflag"], row["l_quantity"]), set()).add(block_of[r])
    assert any(len(b) > 1 for b in seen.values())  # one (key, value) pair in two file blocks: per-block marks would count it twice
    per_key = expected(rows, ["l_returnflag"], "l_quantity")
    assert all(c < sum(1 for r in rows if r["l_returnflag"] == k) for k, c in per_key.items())  # counts below the row counts


@pytest.mark.parametrize("table", LINEITEMS)
def test_counts_by_one_key_with_the_other_aggregates(engine, api, table):
    path = load_golden(table)["paths"]["lineitem"]
    rows = table_rows(path)
    C, F = api.Col, api.F
    rest = [F.sum(C("l_quantity")), F.avg(C("l_extendedprice")), F.min(C("l_discount")), F.max(C("l_tax")), F.count()]
    frame = api.DataFrame().table(path).group_by(C("l_returnflag")).agg(
        F.count_distinct(C("l_quantity")).alias("dq"), *rest[:2], F.count_distinct(C("l_shipmode")).alias("dm"), *rest[2:])
    got = frame.collect()
    want = [expected(rows, ["l_returnflag"], "l_quantity"), expected(rows, ["l_returnflag"], "l_shipmode")]
    assert list(got[0]) == ["l_returnflag", "dq", "sum_l_quantity", "avg_l_extendedprice", "dm", "min_l_discount",
                            "max_l_tax", "count"]
    assert_counts_and_rest(got, ["l_returnflag"], ["dq", "dm"], want,
                           oracle_rows(api.DataFrame().table(path).group_by(C("l_returnflag")).agg(*rest)))
    text = (f"SELECT l_returnflag, COUNT(DISTINCT l_quantity) AS dq, SUM(l_quantity), AVG(l_extendedprice), "
            f"COUNT(DISTINCT l_shipmode) AS dm, MIN(l_discount), MAX(l_tax), COUNT() FROM '{path}' GROUP BY l_returnflag;")
    assert sorted(engine.sql(text).collect(), key=lambda r: r["l_returnflag"]) == sorted(got, key=lambda r: r["l_returnflag"])
    assert frame.collect() == got  # the recording was poisoned, not replayed wrongly
    assert frame.collect() == got


def with_tuple_id(path, keys, folder):
    """The table once more, block for block, with one more INTEGER column ``g`` = the dense id of the row's key tuple: the
    CPU oracle groups by one column only (the idiom of tests/test_gpu_group_by_keys.py).  -> (path, {g: tuple})"""
    from minispark_amd.io import BlockFile

    src = BlockFile(path)
    ids: dict = {}
    g = np.asarray([ids.setdefault(tuple(r[k] for k in keys), len(ids)) for r in table_rows(path)], dtype=np.int32)
    blocks, at = [], 0
    for b, size in enumerate(src.block_rows()):
        blocks.append([*src.read_block_raw(b), g[at: at + size]])
        at += size
    schema = [*src.file_schema, ("g", T.INTEGER)]
    out = str(folder / "keyed.bin")
    BlockFile(out, schema).write_raw_blocks(schema, blocks)
    return out, {v: k for k, v in ids.items()}


@pytest.mark.parametrize("table", LINEITEMS)
def test_counts_by_the_row_form(engine, api, table, tmp_path):
    path = load_golden(table)["paths"]["lineitem"]
    rows = table_rows(path)
    keys = ["l_returnflag", "l_shipmode"]
    text = (f"SELECT l_returnflag, l_shipmode, COUNT(DISTINCT l_quantity) AS dq, SUM(l_quantity), COUNT() FROM '{path}' "
            "GROUP BY (l_returnflag, l_shipmode);")
    got = engine.sql(text).collect()
    keyed, tuples_of = with_tuple_id(path, keys, tmp_path)
    C, F = api.Col, api.F
    by_id = oracle_rows(api.DataFrame().table(keyed).group_by(C("g")).agg(F.sum(C("l_quantity")), F.count()))
    oracle = [{**dict(zip(keys, tuples_of[r["g"]])), **{k: v for k, v in r.items() if k != "g"}} for r in by_id]
    assert_counts_and_rest(got, keys, ["dq"], [expected(rows, keys, "l_quantity")], oracle)
    same = api.DataFrame().table(path).group_by(C("l_returnflag"), C("l_shipmode")).agg(
        F.count_distinct(C("l_quantity")).alias("dq"), F.sum(C("l_quantity")), F.count()).collect()
    assert sorted(map(tuple, (r.values() for r in same))) == sorted(map(tuple, (r.values() for r in got)))


@pytest.mark.parametrize("table", LINEITEMS)
def test_counts_without_group_by_with_a_where_and_of_a_date_part(engine, api, table):
    path = load_golden(table)["paths"]["lineitem"]
    rows = table_rows(path)
    alive = lambda r: r["l_quantity"] > 25  # noqa: E731
    got = engine.sql(f"SELECT COUNT(DISTINCT l_quantity) AS dq, COUNT(DISTINCT l_shipmode) AS dm, COUNT() FROM '{path}';").collect()
    assert got == [{"dq": expected(rows, [], "l_quantity")[None], "dm": expected(rows, [], "l_shipmode")[None],
                    "count": len(rows)}]
    text = (f"SELECT l_returnflag, COUNT(DISTINCT l_quantity) AS dq, COUNT(DISTINCT YEAR(l_shipdate)) AS dy, SUM(l_quantity), "
            f"MAX(l_tax), COUNT() FROM '{path}' WHERE l_quantity > 25 GROUP BY l_returnflag;")
    plain = f"SELECT l_returnflag, SUM(l_quantity), MAX(l_tax), COUNT() FROM '{path}' WHERE l_quantity > 25 GROUP BY l_returnflag;"
    want = [expected(rows, ["l_returnflag"], "l_quantity", alive),
            expected(rows, ["l_returnflag"], lambda r: r["l_shipdate"].year, alive)]
    assert any(want[0][k] < expected(rows, ["l_returnflag"], "l_quantity")[k] for k in want[0])  # the WHERE removes values
    assert_counts_and_rest(engine.sql(text).collect(), ["l_returnflag"], ["dq", "dy"], want, oracle_rows(engine.sql(plain)))
    got = engine.sql(f"SELECT COUNT(DISTINCT YEAR(l_shipdate)) AS dy, COUNT(DISTINCT l_orderkey) AS orders FROM '{path}' "
                     "WHERE l_quantity > 25;").collect()
    assert got == [{"dy": expected(rows, [], lambda r: r["l_shipdate"].year, alive)[None],
                    "orders": expected(rows, [], "l_orderkey", alive)[None]}]
    none_left = f"SELECT l_returnflag, COUNT(DISTINCT l_quantity), COUNT() FROM '{path}' WHERE l_quantity > 1000 GROUP BY l_returnflag;"
    assert engine.sql(none_left).collect() == []
    assert engine.sql(f"SELECT COUNT(DISTINCT l_quantity) FROM '{path}' WHERE l_quantity > 1000;").collect() == []


def test_having_order_by_and_limit_on_the_count(engine, api):
    path = load_golden("q1_multiblock")["paths"]["lineitem"]
    rows = table_rows(path)
    want = expected(rows, ["l_shipmode"], "l_orderkey")
    cut = sorted(want.values())[len(want) // 2]
    text = f"SELECT l_shipmode, COUNT() FROM '{path}' GROUP BY l_shipmode HAVING COUNT(DISTINCT l_orderkey) > {cut};"
    got = engine.sql(text).collect()
    assert 0 < len(got) < len(want)
    assert {r["l_shipmode"] for r in got} == {k for k, c in want.items() if c > cut}
    text = (f"SELECT l_shipmode, COUNT(DISTINCT l_orderkey) AS orders FROM '{path}' GROUP BY l_shipmode "
            "ORDER BY orders DESC, l_shipmode LIMIT 2;")
    top = sorted(want.items(), key=lambda kv: (-kv[1], kv[0]))[:2]
    assert [(r["l_shipmode"], r["orders"]) for r in engine.sql(text).collect()] == top


def test_counts_over_a_join(engine, api):
    paths = load_golden("join_group")["paths"]
    orders, lines = table_rows(paths["orders"]), table_rows(paths["lineitem"])
    priority = {}
    for o in orders:
        priority.setdefault(o["o_orderkey"], []).append(o["o_orderpriority"])
    joined = [{"o_orderpriority": p, **line} for line in lines for p in priority.get(line["l_orderkey"], [])]
    want = expected(joined, ["o_orderpriority"], "l_orderkey")
    assert any(c < sum(1 for r in joined if r["o_orderpriority"] == k) for k, c in want.items())
    C, F = api.Col, api.F

    def frame(*aggs):
        return (api.DataFrame().table(paths["orders"]).join(api.DataFrame().table(paths["lineitem"]),
                                                            on=C("o_orderkey") == C("l_orderkey"), how="inner")
                .group_by(C("o_orderpriority")).agg(*aggs))

    got = frame(F.count_distinct(C("l_orderkey")).alias("orders"), F.sum(C("l_quantity")), F.count()).collect()
    assert_counts_and_rest(got, ["o_orderpriority"], ["orders"], [want],
                           oracle_rows(frame(F.sum(C("l_quantity")), F.count())))
    text = (f"SELECT o_orderpriority, COUNT(DISTINCT l_orderkey) AS orders, SUM(l_quantity), COUNT() FROM '{paths['orders']}' "
            f"JOIN '{paths['lineitem']}' ON o_orderkey=l_orderkey GROUP BY o_orderpriority;")
    assert sorted(map(tuple, (r.values() for r in engine.sql(text).collect()))) == sorted(map(tuple, (r.values() for r in got)))


# ---- through every tier -------------------------------------------------------------------------------------------------
TIER_KEYS = ["k4", "k1000", "k200k"]
TIER_ROWS = 300_000


def tier_frame(api, table, key, distinct=True):
    C, F = api.Col, api.F
    aggs = [F.sum(C("v")), F.count()]
    if distinct:
        aggs.insert(0, F.count_distinct(C("v")).alias("dv"))
    return api.DataFrame().table(table).group_by(C(key)).agg(*aggs)


@pytest.fixture(scope="module")
def tiers(tmp_path_factory):
    """One generated table in five uneven blocks, what Python counts per key, and the oracle's rows without the counts."""
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.io import BlockFile
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    rng = np.random.default_rng(11)
    n = TIER_ROWS
    cols = {"k4": rng.integers(0, 4, n), "k1000": rng.integers(-500, 500, n), "k200k": rng.integers(0, 200_000, n),
            "v": rng.integers(-3, 34, n)}
    schema = [(name, T.INTEGER) for name in cols]
    path = str(tmp_path_factory.mktemp("count_distinct") / "tiers.bin")
    edges = [0, 70_001, 140_000, 141_000, 250_123, n]
    arrays = [cols[name].astype(np.int32) for name in cols]
    BlockFile(path, schema).write_raw_blocks(schema, [[a[lo:hi] for a in arrays] for lo, hi in zip(edges, edges[1:])])
    cpu = api_namespace(lambda: DataFrame(object()), Col, Functions, Lit)
    v = cols["v"].tolist()
    return {"path": path,
            "counts": {key: counts(cols[key].tolist(), v) for key in TIER_KEYS},
            "oracle": {key: oracle_rows(tier_frame(cpu, path, key, distinct=False)) for key in TIER_KEYS}}


def assert_tier_rows(rows, key, tiers):
    want = tiers["counts"][key]
    assert len(rows) == len(want)
    assert all(row["dv"] == want[row[key]] for row in rows)
    assert_rows_match([{k: v for k, v in row.items() if k != "dv"} for row in rows], tiers["oracle"][key])


@pytest.mark.parametrize("key", TIER_KEYS)
def test_the_marks_are_summed_by_every_tier(key, tiers):
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    with HipExecutionEngine(device=0) as e:
        frame = tier_frame(engine_api(e), tiers["path"], key)
        rows = frame.collect()
        tier = "hbm" if e._global_partial else (e.dev.last_scan or {}).get("tier", "private")
        assert tier == {"k4": "private", "k1000": "shared", "k200k": "hbm"}[key]
        assert_tier_rows(rows, key, tiers)
        again = frame.collect()
        assert sorted(map(tuple, (r.values() for r in again))) == sorted(map(tuple, (r.values() for r in rows)))
    assert len(tiers["counts"][key]) > {"k4": 3, "k1000": 999, "k200k": 100_000}[key]
    assert max(tiers["counts"][key].values()) <= 37


@pytest.mark.parametrize("switch", ["HIPSPARK_JIT", "HIPSPARK_SHORT_TAIL"])
def test_the_tiers_with_a_switch_off_in_a_process_of_its_own(switch, tiers, tmp_path):
    out = tmp_path / "rows.json"
    env = dict(os.environ, **{switch: "0"})
    done = subprocess.run([sys.executable, str(ROOT / "tests" / "count_distinct_worker.py"), "tiers", tiers["path"], str(out)],
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, check=False)
    assert done.returncode == 0, done.stdout.decode()[-3000:]
    result = json.loads(out.read_text())
    assert result["switches"]["short_tail"] == (switch != "HIPSPARK_SHORT_TAIL")
    assert (result["switches"]["jit_launches"] == 0) == (switch == "HIPSPARK_JIT")  # the interpreter kernels, or none of them
    for key in TIER_KEYS:
        names = [key, "dv", "sum_v", "count"]
        assert_tier_rows([dict(zip(names, r)) for r in result["rows"][key]], key, tiers)


# ---- refusals on the device ---------------------------------------------------------------------------------------------
def test_a_streamed_scan_with_count_distinct_is_refused_and_runs_without_it():
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from minispark_amd.workloads import engine_api

    path = load_golden("q1_multiblock")["paths"]["lineitem"]
    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: the table streams in several ranges (tests/test_gpu_streaming.py)
        api = engine_api(e)
        C, F = api.Col, api.F
        by_flag = api.DataFrame().table(path).group_by(C("l_returnflag"))
        with pytest.raises(ExecutionError, match=r"COUNT\(DISTINCT\).*HIPSPARK_HBM_BUDGET"):
            by_flag.agg(F.count_distinct(C("l_shipmode")), F.count()).collect()
        plain = api.DataFrame().table(path).group_by(C("l_returnflag")).agg(F.count())
        assert e.streamed_ranges == 0
        assert_rows_match(plain.collect(), oracle_rows(plain))
        assert e.streamed_ranges > 1


def test_a_join_whose_inputs_stream_still_hands_the_marks_the_whole_join():
    """Under a small budget both scan stages of the join read their tables range by range; the mark task is the join
    stage's first consumer, so the probe side is never deferred to a range-by-range join (execution.probe_side_streams):
    the ranges are concatenated, the join runs resident and the marks see every joined row - the counts are the resident
    run's.  The refusal in front of the range-by-range join guards a route this plan cannot take
    (tests/test_count_distinct_cpu.py pins the guard itself)."""
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    paths = load_golden("join_group")["paths"]
    orders, lines = table_rows(paths["orders"]), table_rows(paths["lineitem"])
    priority: dict = {}
    for o in orders:
        priority.setdefault(o["o_orderkey"], []).append(o["o_orderpriority"])
    joined = [{"o_orderpriority": p, **line} for line in lines for p in priority.get(line["l_orderkey"], [])]
    want = expected(joined, ["o_orderpriority"], "l_orderkey")
    with HipExecutionEngine(device=0) as e:
        e.hbm_budget = 2048  # bytes: both tables stream in several ranges
        api = engine_api(e)
        C, F = api.Col, api.F
        frame = (api.DataFrame().table(paths["orders"]).join(api.DataFrame().table(paths["lineitem"]),
                                                             on=C("o_orderkey") == C("l_orderkey"), how="inner")
                 .group_by(C("o_orderpriority")).agg(F.count_distinct(C("l_orderkey")).alias("orders"), F.count()))
        got = frame.collect()
        assert e.streamed_ranges > 2 and e.last_probe_route != "ranges"
    assert {r["o_orderpriority"]: r["orders"] for r in got} == want
    assert {r["o_orderpriority"]: r["count"] for r in got} == counts([r["o_orderpriority"] for r in joined], range(len(joined)))


def test_two_ranks_refuse_on_every_rank_and_go_on(tmp_path):
    out = tmp_path / "ranks.json"
    run_ranks([ROOT / "tests" / "count_distinct_worker.py", "ranks", out])
    results = [json.loads((tmp_path / f"ranks.json.rank{rank}").read_text()) for rank in range(2)]
    assert all("COUNT(DISTINCT) runs on one GPU" in r["refused"] for r in results)
    assert len(results[0]["rows"]) == 3 and results[1]["rows"] == []  # rank 0 owns the result of the query that ran
