"""Joins whose probe (right) side exceeds the HBM budget, in every shape the resident engine answers.  The probe side's
scan stage is either read range by range by the join stage (a byte-table join feeding a GROUP BY, or a join writing the
result file) or streamed through its own scan stage, concatenated and joined resident.  Every case runs twice on one
engine against the Python oracle, proves that the probe side streamed, and pins which of the two routes ran."""

from __future__ import annotations

import random

import numpy as np
import pytest

from tests.conftest import assert_rows_match
from tests.test_gpu_join_dict import _api, _join_queries, _join_tables, _oracle_api

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1


# ---- table makers ------------------------------------------------------------------------------------------------
def _write(path, schema, columns, cuts):
    """columns (numpy arrays or lists of str) split into blocks of the row counts in ``cuts``."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile, StrCol

    blocks, lo = [], 0
    for rows in cuts:
        hi = lo + rows
        blocks.append([StrCol.from_strings(c[lo:hi]) if t == T.STRING else c[lo:hi] for (_, t), c in zip(schema, columns)])
        lo = hi
    assert lo == len(columns[0])
    BlockFile(path).write_raw_blocks(schema, blocks)
    return str(path)


def _keyed_tables(tmp_path, build_keys, probe_keys, seed, tags=None, probe_cuts=None, probe_q=None):
    """dim(d_key, d_tag, d_tag2, d_w) JOIN fact(f_key, f_q, f_p): keys INTEGER (numpy) or STRING (lists).  d_tag2 is a
    second dictionary-coded build column; ``tags`` replaces d_tag's values (e.g. more than 256 of them)."""
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(seed)
    nb, npr = len(build_keys), len(probe_keys)
    kind = T.STRING if isinstance(build_keys, list) else T.INTEGER
    tag = tags if tags is not None else [f"tag-{int(c)}" for c in rng.integers(0, 6, nb)]
    # more values than d_tag: a byte table built for d_tag holds codes that are valid (and wrong) in d_tag2's dictionary
    tag2 = [f"other-{int(c)}" for c in rng.integers(0, 8, nb)]
    w = np.round(rng.uniform(1, 100, nb), 2).astype(np.float32)
    q = probe_q if probe_q is not None else rng.integers(1, 51, npr).astype(np.float32)
    p = (rng.integers(90000, 200001, npr) / 100.0).astype(np.float32)
    dim = _write(tmp_path / "dim.bin", [("d_key", kind), ("d_tag", T.STRING), ("d_tag2", T.STRING), ("d_w", T.FLOAT)],
                 [build_keys, tag, tag2, w], [nb // 2, nb - nb // 2])
    cuts = probe_cuts or [npr // 3, npr // 3, npr - 2 * (npr // 3)]
    fact = _write(tmp_path / "fact.bin", [("f_key", kind), ("f_q", T.FLOAT), ("f_p", T.FLOAT)], [probe_keys, q, p], cuts)
    return dim, fact


def _keyed_group(api, dim, fact, tag="d_tag"):
    C, F = api.Col, api.F
    d = api.DataFrame().table(dim).select(C("d_key"), C(tag))
    f = api.DataFrame().table(fact).select(C("f_key"), C("f_q"), C("f_p"))
    return (d.join(f, on=C("d_key") == C("f_key"), how="inner").group_by(C(tag))
            .agg(F.count().alias("n"), F.sum(C("f_q")).alias("q"), F.max(C("f_p")).alias("hi")))


def _keyed_to_file(api, dim, fact):
    C = api.Col
    d = api.DataFrame().table(dim).select(C("d_key"), C("d_tag"))
    f = api.DataFrame().table(fact).select(C("f_key"), C("f_q"), C("f_p"))
    return (d.join(f, on=C("d_key") == C("f_key"), how="inner").filter(C("f_q") > 10)
            .select(C("d_tag"), C("f_key"), (C("f_p") * 2).alias("twice")))


def _sparse_int_tables(tmp_path):
    """Unique build keys spread over the whole int32 range, the extremes, 0 and -1 (whose Python hash is -2) among
    them; probe keys hit them with duplicates and miss with random keys."""
    rng = np.random.default_rng(41)
    keys = np.unique(rng.integers(INT32_MIN, INT32_MAX, 3000, dtype=np.int64))
    keys = np.unique(np.concatenate([keys, [INT32_MIN, INT32_MAX, 0, -1]])).astype(np.int32)
    rng.shuffle(keys)
    probe = np.concatenate([rng.choice(keys, 10_000), np.repeat(np.array([INT32_MIN, INT32_MAX, 0, -1], np.int32), 50),
                            rng.integers(INT32_MIN, INT32_MAX, 1800, dtype=np.int64).astype(np.int32)])
    rng.shuffle(probe)
    return _keyed_tables(tmp_path, keys, probe, seed=42)


def _string_key_tables(tmp_path):
    """STRING join keys of 17..40 bytes, duplicates on both sides, some sharing a 16-byte prefix; probe misses too."""
    rng = random.Random(43)
    distinct = [f"customer-account-{i:06d}" + "x" * rng.randint(0, 16) for i in range(1200)]
    build = [rng.choice(distinct) for _ in range(1500)]  # ~300 keys twice or more on the build side
    probe = [rng.choice(distinct) if rng.random() < 0.9 else f"customer-account-{rng.randint(0, 10**6):06d}-miss"
             for _ in range(9000)]
    return _keyed_tables(tmp_path, build, probe, seed=44)


def _chain_tables(tmp_path):
    """customers(c_custkey, c_segment) <- orders(o_orderkey, o_custkey, o_orderpriority) <- lineitem (three blocks)."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.workloads import PRIORITIES, order_key

    rng = np.random.default_rng(45)
    n_cust, n_orders, n_li = 300, 2000, 15_000
    ckey = rng.permutation(n_cust).astype(np.int32) * 3 + 1
    seg = [["AUTOMOBILE", "BUILDING", "MACHINERY", "HOUSEHOLD"][int(c)] for c in rng.integers(0, 4, n_cust)]
    okey = np.array([order_key(int(o)) for o in rng.permutation(n_orders)], np.int32)
    ocust = (rng.integers(0, int(n_cust * 1.1), n_orders) * 3 + 1).astype(np.int32)  # some orders without a customer
    prio = [PRIORITIES[int(c)] for c in rng.integers(0, 5, n_orders)]
    lkey = np.array([order_key(int(o)) for o in rng.integers(0, int(n_orders * 1.2), n_li)], np.int32)
    qty = rng.integers(1, 51, n_li).astype(np.float32)
    price = (qty * rng.integers(90000, 200001, n_li) / 100.0).astype(np.float32)
    cust = _write(tmp_path / "cust.bin", [("c_custkey", T.INTEGER), ("c_segment", T.STRING)], [ckey, seg], [n_cust])
    orders = _write(tmp_path / "orders.bin", [("o_orderkey", T.INTEGER), ("o_custkey", T.INTEGER), ("o_orderpriority", T.STRING)],
                    [okey, ocust, prio], [n_orders // 2, n_orders - n_orders // 2])
    li = _write(tmp_path / "lineitem.bin", [("l_orderkey", T.INTEGER), ("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT)],
                [lkey, qty, price], [5000, 5000, 5000])
    return cust, orders, li


def _chain(api, cust, orders, li, to_file):
    C, F = api.Col, api.F
    c = api.DataFrame().table(cust).select(C("c_custkey"), C("c_segment"))
    o = api.DataFrame().table(orders).select(C("o_orderkey"), C("o_custkey"), C("o_orderpriority"))
    l = api.DataFrame().table(li).select(C("l_orderkey"), C("l_quantity"), C("l_extendedprice"))
    joined = c.join(o.join(l, on=C("o_orderkey") == C("l_orderkey"), how="inner"), on=C("c_custkey") == C("o_custkey"),
                    how="inner")
    if to_file:
        return joined.filter(C("l_quantity") > 40).select(C("c_segment"), C("o_orderpriority"), C("l_orderkey"),
                                                          C("l_extendedprice"))
    return joined.group_by(C("c_segment")).agg(F.count().alias("n"), F.sum(C("l_quantity")).alias("q"))


def _uneven_tables(tmp_path, seed, cuts, empty_first=False):
    """orders (1000 rows) + lineitem in blocks of ``cuts`` rows; with ``empty_first`` every l_quantity of the first
    block is <= 10 and every other one > 10."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.workloads import PRIORITIES, order_key

    rng = np.random.default_rng(seed)
    n_orders, n_li = 1000, sum(cuts)
    okey = np.array([order_key(int(o)) for o in rng.permutation(n_orders)], np.int32)
    prio = [PRIORITIES[int(c)] for c in rng.integers(0, 5, n_orders)]
    total = np.round(rng.uniform(1, 500, n_orders), 2).astype(np.float32)
    lkey = np.array([order_key(int(o)) for o in rng.integers(0, int(n_orders * 1.25), n_li)], np.int32)
    qty = rng.integers(11, 51, n_li).astype(np.float32)
    if empty_first:
        qty[: cuts[0]] = rng.integers(1, 11, cuts[0]).astype(np.float32)
    price = (qty * rng.integers(90000, 200001, n_li) / 100.0).astype(np.float32)
    orders = _write(tmp_path / "orders.bin", [("o_orderkey", T.INTEGER), ("o_orderpriority", T.STRING), ("o_totalprice", T.FLOAT)],
                    [okey, prio, total], [n_orders // 2, n_orders - n_orders // 2])
    li = _write(tmp_path / "lineitem.bin", [("l_orderkey", T.INTEGER), ("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT)],
                [lkey, qty, price], cuts)
    return orders, li


def _orders_lineitem_to_file(api, orders, lineitem):
    C = api.Col
    o = api.DataFrame().table(orders).select(C("o_orderkey"), C("o_orderpriority"))
    li = api.DataFrame().table(lineitem).select(C("l_orderkey"), C("l_quantity"), C("l_extendedprice"))
    return (o.join(li, on=C("o_orderkey") == C("l_orderkey"), how="inner").filter(C("l_quantity") > 10)
            .select(C("o_orderpriority"), C("l_orderkey"), (C("l_extendedprice") * 2).alias("twice")))


# ---- the matrix --------------------------------------------------------------------------------------------------
def _case(name, tmp_path):
    """-> (query builder taking an api, HBM budget in bytes, route, probe ranges per run at least, max_ulps, flips)."""
    if name in ("build_side_argument", "dup_build_keys", "projection_before_group_by", "float_group_key"):
        orders, li = _join_tables(tmp_path, 3000, 24_000, seed=51, dup=name == "dup_build_keys")
        if name == "build_side_argument":
            return (lambda api: _join_queries(api, orders, li)["filtered_with_build_side_argument"]), 150_000, "resident", 3, 1, 2
        if name == "dup_build_keys":
            return (lambda api: _join_queries(api, orders, li)["config4"]), 150_000, "resident", 3, 1, 2

        def build(api):
            C, F = api.Col, api.F
            o = api.DataFrame().table(orders).select(C("o_orderkey"), C("o_orderpriority"), C("o_totalprice"))
            l = api.DataFrame().table(li).select(C("l_orderkey"), C("l_quantity"), C("l_extendedprice"))
            j = o.join(l, on=C("o_orderkey") == C("l_orderkey"), how="inner")
            if name == "float_group_key":  # a FLOAT build-side key: no dictionary code for the byte table
                return j.group_by(C("o_totalprice")).agg(F.count().alias("n"), F.sum(C("l_quantity")).alias("q"))
            return (j.select((C("l_extendedprice") * 2).alias("x"), C("o_orderpriority")).group_by(C("o_orderpriority"))
                    .agg(F.sum(C("x")).alias("sx"), F.count().alias("n")))
        return build, 150_000, "resident", 3, 1, 2
    if name in ("sparse_int_keys_group", "sparse_int_keys_to_file"):
        dim, fact = _sparse_int_tables(tmp_path)
        if name.endswith("group"):
            return (lambda api: _keyed_group(api, dim, fact)), 100_000, "resident", 3, 1, 2
        return (lambda api: _keyed_to_file(api, dim, fact)), 100_000, "ranges", 3, 0, 0
    if name in ("string_keys_group", "string_keys_to_file"):
        dim, fact = _string_key_tables(tmp_path)
        if name.endswith("group"):
            return (lambda api: _keyed_group(api, dim, fact)), 250_000, "resident", 3, 1, 2
        return (lambda api: _keyed_to_file(api, dim, fact)), 250_000, "ranges", 3, 0, 0
    if name == "many_string_group_keys":  # 1500 distinct build-side strings: the column stays plain
        rng = np.random.default_rng(46)
        keys = rng.permutation(1500).astype(np.int32) * 2
        dim, fact = _keyed_tables(tmp_path, keys, rng.choice(keys, 12_000).astype(np.int32), seed=47,
                                  tags=[f"group-{i:05d}" for i in range(1500)])
        return (lambda api: _keyed_group(api, dim, fact)), 100_000, "resident", 3, 1, 2
    if name in ("chain_group", "chain_to_file"):
        cust, orders, li = _chain_tables(tmp_path)
        return (lambda api: _chain(api, cust, orders, li, name.endswith("to_file"))), 100_000, "resident", 3, 0 if name.endswith("to_file") else 1, 2
    raise KeyError(name)


MATRIX = ["build_side_argument", "dup_build_keys", "sparse_int_keys_group", "sparse_int_keys_to_file", "string_keys_group",
          "string_keys_to_file", "projection_before_group_by", "many_string_group_keys", "float_group_key", "chain_group",
          "chain_to_file"]


def _check_route(engine, route, runs):
    """After run number ``runs``: 'ranges' - the join stage read the deferred probe side range by range, on every run;
    'resident' - the probe side was streamed through its scan stage, concatenated and joined resident."""
    assert engine.last_probe_route == route
    if route == "ranges":
        assert engine.streamed_join_fallbacks == 0
    else:
        assert engine.streamed_join_fallbacks >= runs
    assert engine._join8_reuse is None


@pytest.mark.parametrize("name", MATRIX)
def test_streamed_probe_side_matches_the_oracle(tmp_path, name):
    from minispark_amd.execution import HipExecutionEngine
    from oracle.py_engine import run_query

    build, budget, route, ranges, max_ulps, max_flips = _case(name, tmp_path)
    want = run_query(build(_oracle_api()).task)
    assert len(want) > 3
    with HipExecutionEngine(device=0) as engine:
        engine.hbm_budget = budget
        frame = build(_api(engine))
        for run in range(2):
            assert assert_rows_match(frame.collect(), want, max_ulps=max_ulps) <= max_flips
            assert engine.streamed_ranges >= ranges * (run + 1), "the probe side must not fit the budget"
            _check_route(engine, route, run + 1)


def test_probe_side_group_key_outgrows_its_table_on_a_later_range(tmp_path):
    """GROUP BY a probe-side INTEGER key through the byte-table join: the first range holds 8 distinct keys (within
    the starting per-JoinJob tables), the later ones over a thousand.  The overflow of a later range is noticed at the
    end of the query and the dictionaries grow until the fused probe's tiers cannot hold them: like the resident engine
    (_no_join8 / _no_short_tail), the query then runs without the byte table - here with its probe side joined
    resident."""
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import order_key
    from oracle.py_engine import run_query

    orders, li = _uneven_tables(tmp_path, 52, [6000, 6000, 6000])
    # rewrite lineitem: block 0 references 8 orders only
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(53)
    few = np.array([order_key(o) for o in range(8)], np.int32)
    lkey = np.concatenate([rng.choice(few, 6000), np.array([order_key(int(o)) for o in rng.integers(0, 1250, 12_000)], np.int32)])
    qty = rng.integers(1, 51, 18_000).astype(np.float32)
    price = (qty * rng.integers(90000, 200001, 18_000) / 100.0).astype(np.float32)
    li = _write(tmp_path / "lineitem.bin", [("l_orderkey", T.INTEGER), ("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT)],
                [lkey, qty, price], [6000, 6000, 6000])
    assert len(set(lkey[:6000].tolist())) == 8 and len(set(lkey[6000:12_000].tolist())) > 900
    want = run_query(_join_queries(_oracle_api(), orders, li)["probe_side_int_key"].task)
    assert len(want) > 900
    with HipExecutionEngine(device=0) as engine:
        engine.hbm_budget = 100_000  # lineitem: 72 KB blocks, one per range; orders stays resident
        frame = _join_queries(_api(engine), orders, li)["probe_side_int_key"]
        for _ in range(2):
            assert assert_rows_match(frame.collect(), want, max_ulps=1) <= 2
        assert engine.group_cap_hint > 4, "a later range overflowed the starting capacity"
        assert engine.streamed_ranges >= 6 and engine.fused_probes >= 1
        assert engine._no_join8 or engine._no_short_tail, "the fused probe's tier gave up on this GROUP BY"
        _check_route(engine, "resident", 2)


def test_both_sides_beyond_the_budget(tmp_path):
    """orders streams through its own scan stage, lineitem is the deferred probe side."""
    from minispark_amd.execution import HipExecutionEngine
    from oracle.py_engine import run_query

    orders, li = _join_tables(tmp_path, 6000, 24_000, seed=54)
    want = run_query(_join_queries(_oracle_api(), orders, li)["config4"].task)
    with HipExecutionEngine(device=0) as engine:
        engine.hbm_budget = 40_000  # orders' two blocks are larger than a range too
        frame = _join_queries(_api(engine), orders, li)["config4"]
        for run in range(2):
            assert assert_rows_match(frame.collect(), want, max_ulps=1) <= 2
            assert engine.streamed_ranges >= 5 * (run + 1)
            # the streamed build side is not dictionary-coded: the byte table cannot carry its GROUP BY key
            _check_route(engine, "resident", run + 1)


@pytest.mark.parametrize("shape", ["group_by", "to_file"])
@pytest.mark.parametrize("tables", ["uneven_ranges", "first_range_filtered_out"])
def test_ranges_of_unequal_size_and_empty_ranges(tmp_path, tables, shape):
    """Budget 50 000 B, lineitem blocks of 12 B rows: ranges of 2, 1 and 3 blocks with a short last block - or, with
    every row of the first range filtered out, an empty range followed by full ones.  GROUP BY: the raw per-JoinJob
    tables are added across ranges; file: the append-merge rule keeps full blocks and one short last block."""
    from minispark_amd import constants
    from minispark_amd import table as tbl
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.plan import PhysicalPlan
    from oracle import blockfile as bfio
    from oracle.py_engine import run_query

    if tables == "uneven_ranges":
        cuts, ranges = [1000, 1000, 1800, 600, 600, 300], [[0, 1], [2], [3, 4, 5]]
        orders, li = _uneven_tables(tmp_path, 55, cuts)
    else:
        cuts, ranges = [2000, 2000, 2000], [[0], [1], [2]]
        orders, li = _uneven_tables(tmp_path, 56, cuts, empty_first=True)
    query = ((lambda api: _join_queries(api, orders, li)["filtered_on_the_probe_side"]) if shape == "group_by"
             else (lambda api: _orders_lineitem_to_file(api, orders, li)))
    want = run_query(query(_oracle_api()).task)
    assert len(want) >= 5
    with HipExecutionEngine(device=0) as engine:
        engine.hbm_budget = 50_000
        frame = query(_api(engine))
        (scan,) = [st for st in PhysicalPlan.generate_physical_plan(frame.task).stages
                   if str(getattr(st.producer, "file_path", "")) == li]
        assert tbl.referenced_block_bytes(engine._table(li), [0, 1, 2]) == [12 * c for c in cuts]
        assert engine._stream_ranges(scan.producer, list(scan.consumers)) == ranges
        if shape == "group_by":
            for run in range(2):
                assert assert_rows_match(frame.collect(), want, max_ulps=1) <= 2
                _check_route(engine, "ranges", run + 1)
            assert engine.dev.last_join["mode"] == "byte table"
        else:
            constants.ROWS_PER_BLOCK = 700
            try:
                for _ in range(2):
                    results = engine.execute_full_task(frame.task)
                    (path,) = [f.file_path for r in results for f in r.output_files]
                    _, blocks = bfio.read_blockfile(path)
                    sizes = [len(b[0]) for b in blocks]
                    assert all(sz == 700 for sz in sizes[:-1]) and 0 < sizes[-1] <= 700
                    rows = list(engine.collect_results(results))
                    assert assert_rows_match(rows, want, max_ulps=0) == 0
                    _check_route(engine, "ranges", 1)
            finally:
                constants.ROWS_PER_BLOCK = 2 * 1024 * 1024
        assert engine.streamed_ranges == 2 * len(ranges)


def test_a_failed_streamed_query_leaves_no_byte_table_behind(tmp_path, monkeypatch):
    """A device error on the second range of a streamed byte-table join reaches the caller; the engine keeps no byte
    table of that query, so a later fused join over the same build column with ANOTHER payload column (d_tag2 instead
    of d_tag) answers with its own codes."""
    from minispark_amd.device import DeviceError
    from minispark_amd.execution import ExecutionError, HipExecutionEngine
    from oracle.py_engine import run_query

    rng = np.random.default_rng(57)
    keys = rng.permutation(2000).astype(np.int32) + 100
    dim, fact = _keyed_tables(tmp_path, keys, rng.choice(keys, 12_000).astype(np.int32), seed=58)
    with HipExecutionEngine(device=0) as engine:
        engine.hbm_budget = 100_000
        real, calls = engine.dev.aggregate_join8, []

        def failing(*args, **kwargs):
            calls.append(1)
            if len(calls) == 2:
                raise DeviceError("injected: the second range's aggregate failed")
            return real(*args, **kwargs)

        monkeypatch.setattr(engine.dev, "aggregate_join8", failing)
        with pytest.raises(ExecutionError, match="injected") as info:
            _keyed_group(_api(engine), dim, fact).collect()
        assert isinstance(info.value.__cause__, DeviceError) and len(calls) == 2
        assert engine._join8_reuse is None
        monkeypatch.setattr(engine.dev, "aggregate_join8", real)

        engine.hbm_budget = None  # resident: the fused probe builds a byte table of its own
        want = run_query(_keyed_group(_oracle_api(), dim, fact, tag="d_tag2").task)
        assert assert_rows_match(_keyed_group(_api(engine), dim, fact, tag="d_tag2").collect(), want, max_ulps=1) <= 2
        assert engine.dev.last_join["mode"] == "byte table"
