"""The shared-dictionary aggregation tier (tens to thousands of groups per unit; LDS atomics) against the oracle.
Additions of a group happen in hardware order there, so FLOAT SUM / AVG results may differ from the reference's sequential
sums at an f32 rounding boundary: at most one ulp, and rarely (the test bounds the number of such values).  MIN, MAX, COUNT
and every INTEGER column do not depend on the order and are compared exactly."""

from __future__ import annotations

import random
from ctypes import c_int32 as C_int32

import numpy as np
import pytest

from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu

WORDS = [f"key-{i:04d}-{'x' * (i % 9)}" for i in range(400)]  # 8..16 bytes: long keys compare bytes ("hashed" mode)


@pytest.fixture(scope="module")
def engine():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine(0) as e:
        yield e


def _assert_match(got, want, loose):
    """assert_rows_match with the one-ulp allowance, then every column outside `loose` (the FLOAT SUM / AVG columns) exactly,
    row by row under the group key (the first column).  -> the number of values an ulp apart"""
    flips = assert_rows_match(got, want, max_ulps=1)
    if not want:  # (a filter that keeps no row: the row counts already agree)
        return flips
    key = next(iter(want[0]))
    by_key = {row[key]: row for row in want}
    assert len(by_key) == len(want)
    for row in got:
        for name, value in row.items():
            if name not in loose:
                other = by_key[row[key]][name]
                assert type(value) is type(other) and value == other, f"{key}={row[key]!r} {name}: {value!r} != {other!r}"
    return flips


LOOSE = {"int key, 1400 groups": {"sf", "av"}, "long string key, 400 groups, filtered": {"x"}, "computed int key": {"sf"}}


def _table(path, n, blocks, seed):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile, StrCol

    rng = np.random.default_rng(seed)
    k = rng.integers(-700, 700, n).astype(np.int32)
    s = [WORDS[i] for i in rng.integers(0, len(WORDS), n)]
    f = rng.normal(0, 1e3, n).astype(np.float32)
    g = rng.uniform(0, 1, n).astype(np.float32)
    i = rng.integers(-10**5, 10**5, n).astype(np.int32)
    schema = [("k", T.INTEGER), ("s", T.STRING), ("f", T.FLOAT), ("g", T.FLOAT), ("i", T.INTEGER)]
    bounds = np.linspace(0, n, blocks + 1).astype(int)
    out = []
    for lo, hi in zip(bounds, bounds[1:]):
        out.append([k[lo:hi], StrCol.from_strings(s[lo:hi]), f[lo:hi], g[lo:hi], i[lo:hi]])
    BlockFile(path).write_raw_blocks(schema, out)


def _queries(api, path):
    C, F, Lit = api.Col, api.F, api.Lit
    t = lambda: api.DataFrame().table(path)  # noqa: E731
    return {
        "int key, 1400 groups": t().group_by(C("k")).agg(F.sum(C("f")).alias("sf"), F.sum(C("i")).alias("si"), F.count(),
                                                          F.min(C("f")).alias("mn"), F.max(C("i")).alias("mx"),
                                                          F.avg(C("g")).alias("av")),
        "long string key, 400 groups, filtered": t().filter(C("g") > 0.25).group_by(C("s")).agg(
            F.sum(C("f") * (Lit(1) - C("g"))).alias("x"), F.count(), F.min(C("i")).alias("mn")),
        "computed int key": t().select((C("k") % 97).alias("m"), C("f"), C("i")).group_by(C("m")).agg(
            F.sum(C("f")).alias("sf"), F.max(C("f")).alias("mx"), F.count()),
    }


def test_many_group_queries_match_the_oracle(engine, tmp_path):
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from oracle.py_engine import run_query
    from tests.queries import api_namespace

    path = tmp_path / "t.bin"
    _table(path, 60_000, 4, 11)
    ours = _queries(api_namespace(lambda: DataFrame(engine), Col, Functions, Lit), str(path))
    oracle = _queries(api_namespace(lambda: DataFrame(object()), Col, Functions, Lit), str(path))
    for name in ours:
        want = run_query(oracle[name].task)
        for _run in range(2):
            got = ours[name].collect()
            flips = _assert_match(got, want, LOOSE[name])
            assert flips <= 3, f"{name}: {flips} values moved across an f32 rounding boundary"
        assert engine.dev.last_scan["tier"] == "shared", name
        assert engine.dev.last_scan["wg_threads"] == 1024


def test_the_interpreter_kernels_of_the_shared_tier_match_the_oracle(tmp_path):
    """Without the run-time compiler (HIPSPARK_JIT=0, or hiprtc missing) the shared tier runs its ahead-of-time
    interpreter kernels k_agg_shared<...>: 512 lanes wide for expression stacks of depth <= 4, 256 lanes for depth 8 and for
    long string keys ("hashed") - round 3 ran them at 1024 lanes with the stack in scratch memory.  Same chunks, same
    results: the three query shapes (packed INTEGER key, 8-16 byte string key, computed key) against the oracle."""
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.sql import Col, Functions, Lit
    from oracle.py_engine import run_query
    from tests.queries import api_namespace

    path = tmp_path / "t.bin"
    _table(path, 60_000, 4, 12)
    oracle = _queries(api_namespace(lambda: DataFrame(object()), Col, Functions, Lit), str(path))
    with HipExecutionEngine(0) as e:
        e.dev.lib.hs_jit_set_enabled(0)
        try:
            ours = _queries(api_namespace(lambda: DataFrame(e), Col, Functions, Lit), str(path))
            stats = (C_int32 * 3)()
            e.dev.lib.hs_jit_stats(stats)
            launches_before = stats[1]
            for name in ours:
                want = run_query(oracle[name].task)
                for _run in range(2):
                    assert _assert_match(ours[name].collect(), want, LOOSE[name]) <= 3, name
                assert e.dev.last_scan["tier"] == "shared", name
            e.dev.lib.hs_jit_stats(stats)
            assert stats[1] == launches_before, "no compiled program may have run"
        finally:
            e.dev.lib.hs_jit_set_enabled(1)


def test_counts_and_integer_sums_are_exact_at_scale(engine, tmp_path):
    """2 M rows, 5000 groups: COUNT and INTEGER SUM / MIN / MAX are order-independent and must be exact."""
    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.device import DCol
    from minispark_amd.io import BlockFile
    from minispark_amd.sql import Col, Functions as F
    from minispark_amd.table import DeviceTable

    import torch

    n = 2_000_000
    rng = np.random.default_rng(5)
    k = rng.integers(0, 5000, n).astype(np.int32)
    v = rng.integers(-1000, 1000, n).astype(np.int32)
    schema = [("k", T.INTEGER), ("v", T.INTEGER)]
    path = tmp_path / "big.bin"
    BlockFile(path, schema).write_rows([])
    sizes = [700_000, 700_000, 600_000]
    table = DeviceTable(path, schema, sizes, {}, ())
    table.columns[0] = DCol(hs.I32, engine.dev.to_device(k, torch.int32), n)
    table.columns[1] = DCol(hs.I32, engine.dev.to_device(v, torch.int32), n)
    engine.attach_device_table(path, table)
    q = DataFrame(engine).table(str(path)).group_by(Col("k")).agg(F.count(), F.sum(Col("v")).alias("s"),
                                                                   F.min(Col("v")).alias("mn"), F.max(Col("v")).alias("mx"))
    rows = {r["k"]: r for r in q.collect()}
    assert engine.dev.last_scan["tier"] == "shared"
    assert len(rows) == len(np.unique(k))
    cnt = np.bincount(k, minlength=5000)
    sums = np.bincount(k, weights=v.astype(np.float64), minlength=5000)
    for key in random.Random(1).sample(sorted(rows), 300):
        sel = v[k == key]
        r = rows[key]
        assert (r["count"], r["s"], r["mn"], r["mx"]) == (int(cnt[key]), int(sums[key]), int(sel.min()), int(sel.max()))


def _wide_table(path, n, blocks, seed):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile, StrCol

    rng = np.random.default_rng(seed)
    cols = {
        "h": rng.integers(0, int(rng.choice([40, 300, 3000, 9000])), n).astype(np.int32),
        "u": [WORDS[i] for i in rng.integers(0, int(rng.choice([30, 400])), n)],
        "f": rng.normal(0, 1e3, n).astype(np.float32),
        "g": rng.uniform(0, 1, n).astype(np.float32),
        "i": rng.integers(-10**5, 10**5, n).astype(np.int32),
    }
    schema = [("h", T.INTEGER), ("u", T.STRING), ("f", T.FLOAT), ("g", T.FLOAT), ("i", T.INTEGER)]
    bounds = sorted({0, n, *rng.integers(1, n, blocks - 1).tolist()})
    out = []
    for lo, hi in zip(bounds, bounds[1:]):
        out.append([cols["h"][lo:hi], StrCol.from_strings(cols["u"][lo:hi]), cols["f"][lo:hi], cols["g"][lo:hi], cols["i"][lo:hi]])
    BlockFile(path).write_raw_blocks(schema, out)


def _wide_query(rng: random.Random, api, path):
    return _wide_query_and_loose(rng, api, path)[0]


def _wide_query_and_loose(rng: random.Random, api, path):
    """-> (the query, the names of its FLOAT SUM / AVG columns)"""
    C, F, Lit = api.Col, api.F, api.Lit
    df = api.DataFrame().table(path)
    if rng.random() < 0.5:
        df = df.filter(rng.choice([C("g") > 0.3, C("i") % 3 != 0, (C("f") < 500.0) & (C("g") <= 0.9), C("u") >= "key-0100"]))
    key = rng.choice(["h", "u", "m", "hu"])
    if key == "m":
        df = df.select((C("h") % rng.choice([17, 97, 1013])).alias("m"), C("f"), C("g"), C("i"))
    elif key == "hu":
        df = df.select((C("u") + "/" + C("u")).alias("hu"), C("f"), C("g"), C("i"))
    pool = [lambda: F.sum(C("f")), lambda: F.sum(C("i")), lambda: F.min(C("f")), lambda: F.max(C("i")), lambda: F.avg(C("g")),
            lambda: F.sum(C("f") * (Lit(1) - C("g"))), lambda: F.min(C("i")), lambda: F.max(C("g"))]
    picked = rng.sample(range(len(pool)), rng.randint(1, 4))  # (the same draws as a sample of the pool itself)
    aggs = [pool[p]().alias(f"a{n}") for n, p in enumerate(picked)]
    if rng.random() < 0.7:
        aggs.append(F.count())
    loose = {f"a{n}" for n, p in enumerate(picked) if p in (0, 4, 5)}  # FLOAT SUM / AVG: the order of additions shows
    return df.group_by(C(key)).agg(*aggs), loose


_WIDE_FIRST = int(__import__("os").environ.get("HIPSPARK_WIDE_FIRST", "0"))


@pytest.mark.parametrize("seed", list(range(_WIDE_FIRST, _WIDE_FIRST + int(__import__("os").environ.get("HIPSPARK_WIDE_SEEDS", "12")))))
def test_random_many_group_queries_match_the_oracle(engine, tmp_path, seed):
    """Random GROUP BY queries whose keys have tens to thousands of values (int, long strings, computed int and
    computed string keys), random filters and aggregates, ragged blocks: private tables, the shared dictionary and
    the HBM tier, whichever the capacities end up choosing, against the oracle."""
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from oracle.py_engine import run_query
    from tests.queries import api_namespace

    rng = random.Random(900 + seed)
    path = tmp_path / "w.bin"
    _wide_table(path, rng.choice([5_000, 20_000, 50_000]), rng.choice([1, 3, 7]), seed)
    want = run_query(_wide_query(random.Random(seed), api_namespace(lambda: DataFrame(object()), Col, Functions, Lit), str(path)).task)
    frame, loose = _wide_query_and_loose(random.Random(seed), api_namespace(lambda: DataFrame(engine), Col, Functions, Lit), str(path))
    for _ in range(2):
        flips = _assert_match(frame.collect(), want, loose)
        assert flips <= 3


def _blocks_table(path, blocks, rows_per_block, groups, seed):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile

    rng = np.random.default_rng(seed)
    n = blocks * rows_per_block
    k = rng.integers(0, groups, n).astype(np.int32)
    f = rng.normal(0, 1e3, n).astype(np.float32)
    BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("f", T.FLOAT)],
                                     [[k[b * rows_per_block:(b + 1) * rows_per_block], f[b * rows_per_block:(b + 1) * rows_per_block]]
                                      for b in range(blocks)])


@pytest.mark.parametrize(("groups", "on_chip"), [(50, True), (3000, False)])
def test_final_merge_tier_follows_the_real_number_of_partial_rows(tmp_path, groups, on_chip):
    """The shared tier hands its partial rows over densely with only an UPPER BOUND of their number on the host (units x
    table capacity).  The on-chip merge runs with as many rows as LDS holds: 30 units x 50 groups = 1 500 rows fit (the
    query is then recorded and replayed), 30 x 3 000 = 90 000 raise HS_FLAG_MERGE_ROWS and the query moves to the HBM-tier
    merge - never because of the bound alone, and never because the PER-UNIT dictionaries had to grow on the way."""
    from minispark_amd import constants
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.sql import Col, Functions as F
    from oracle.py_engine import run_query

    constants.SHUFFLE_FOLDER = tmp_path / "shuffle"
    path = tmp_path / "b.bin"
    _blocks_table(path, 30, 4000, groups, groups)

    def build(engine):
        return DataFrame(engine).table(str(path)).group_by(Col("k")).agg(F.sum(Col("f")).alias("s"), F.count(), F.max(Col("f")).alias("m"))

    want = run_query(build(object()).task)
    with HipExecutionEngine(0) as engine:
        frame = build(engine)
        for _ in range(5):
            flips = _assert_match(frame.collect(), want, {"s"})
            assert flips <= 3
        assert engine.dev.last_scan["tier"] == "shared"
        assert bool(engine._global_merge) != on_chip
        assert not engine._caps["merge_overflowed"]
        if on_chip:
            assert engine.replays >= 1


def test_computed_units_at_the_c_abi_with_every_buffer_sized_from_the_geometry(engine):
    """hs_agg_shared_units called directly: two chunks, three unit tables, rows with unit id 0xff (they take no part).
    Chunk table, outputs and workspace are sized from hs_agg_shared_units_geom alone - the contract of that entry.
    Per (unit, key): INTEGER MIN exactly, the FLOAT sum to 1e-12 relative (the values are quarters, so every order of
    additions and the rounding to f32 give the same number; the tier promises ~1e-13)."""
    import ctypes as C

    import torch

    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.sql import Col, Functions as F

    dev, lib = engine.dev, hs.load_library()
    n, tables = 65536 + 4100, 3
    rng = np.random.default_rng(19)
    k = rng.integers(0, 5, n).astype(np.int32) * 1000 - 7
    f = (rng.integers(-4000, 4000, n) / 4).astype(np.float32)
    i = rng.integers(-10**6, 10**6, n).astype(np.int32)
    unit = rng.integers(0, tables + 1, n).astype(np.uint8)
    unit[unit == tables] = 0xFF
    schema = [("k", T.INTEGER), ("f", T.FLOAT), ("i", T.INTEGER)]
    low = lower_aggregate(schema, [hs.I32, hs.F32, hs.I32], [], Col("k"), [F.sum(Col("f")).alias("s"), F.min(Col("i")).alias("m")])
    host = [k, f, i]
    tensors = [torch.from_numpy(host[c]).to(dev.device) for c in low.program.columns] + [torch.from_numpy(unit).to(dev.device)]
    n_cols = len(tensors)
    cols = (hs.hs_col * n_cols)()
    for slot, t in enumerate(tensors):
        cols[slot].kind = hs.U8 if slot == n_cols - 1 else [hs.I32, hs.F32, hs.I32][low.program.columns[slot]]
        cols[slot].fixed_len, cols[slot].data = -1, t.data_ptr()
    prog, spec = low.program.to_struct(), low.spec()
    n_acc = spec.n_acc
    geom = hs.hs_agg_geom()
    hs.check(lib.hs_agg_shared_units_geom(n, tables, n_acc, 16, 0, C.byref(geom)), "hs_agg_shared_units_geom")
    assert geom.n_chunks == 2 and geom.pad >= 16
    bounds = (C.c_int64 * 2)(0, n)
    chunks = np.zeros((geom.n_chunks, 4), dtype=np.int64)
    chunk0 = np.zeros(2, dtype=np.int64)
    hs.check(lib.hs_agg_partial_chunks(bounds, 1, C.byref(geom), chunks.ctypes.data_as(C.POINTER(hs.hs_chunk)),
                                       chunk0.ctypes.data_as(C.POINTER(C.c_int64))), "hs_agg_partial_chunks")
    d_chunks = torch.from_numpy(chunks.reshape(-1)).to(dev.device)
    slots = tables * geom.pad
    rep = torch.full((slots,), -7, dtype=torch.int64, device=dev.device)
    acc = torch.zeros(slots * n_acc, dtype=torch.int64, device=dev.device)
    ngroups = torch.full((tables,), -7, dtype=torch.int32, device=dev.device)
    ws = torch.zeros(geom.ws_bytes, dtype=torch.uint8, device=dev.device)
    dev.reset_flags()
    hs.check(lib.hs_agg_shared_units(dev.stream, cols, n_cols, low.key_slot, n_cols - 1, tables, C.byref(prog), C.byref(spec),
                                     d_chunks.data_ptr(), C.byref(geom), rep.data_ptr(), acc.data_ptr(), ngroups.data_ptr(),
                                     ws.data_ptr(), dev.flags.data_ptr(), None, None), "hs_agg_shared_units")
    assert dev.read_flags() == 0
    rep, acc, ngroups = rep.cpu().numpy().reshape(tables, geom.pad), acc.cpu().numpy().reshape(tables, geom.pad, n_acc), ngroups.cpu().numpy()
    a_sum, a_min = low.agg_to_acc
    for u in range(tables):
        got = {int(k[r]): (acc[u, s, a_sum : a_sum + 1].view(np.float64)[0], int(acc[u, s, a_min]))
               for s, r in enumerate(rep[u]) if r >= 0}
        assert ngroups[u] == len(got) == 5, (u, ngroups[u], sorted(got))
        for key, (s, m) in got.items():
            rows = (unit == u) & (k == key)
            want = float(f[rows].astype(np.float64).sum())
            assert m == int(i[rows].min()), (u, key)
            assert abs(s - want) <= 1e-12 * abs(want), (u, key, s, want)
