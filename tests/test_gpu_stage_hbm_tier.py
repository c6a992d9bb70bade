"""The HBM (radix) aggregation tier behind the native scan stage (hs_stage_set_hbm_tier, NativeStage(hbm_tier=True)): a GROUP BY
of any cardinality through hs_stage_run alone - row-forming pass (hs_agg_rows), radix partial aggregate per file block, radix
merge, projection, rounding - against the Python oracle at 0 ulp: the radix tier folds every group's values in ascending row
order, the merge folds the partial rows in block order and cells are computed per row in fp64, as the reference does."""

from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu


def _api():
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    return api_namespace(lambda: DataFrame(object()), Col, Functions, Lit)


def _too_many(tmp_path):
    """The `too_many` table and query of tests/test_gpu_stage_abi.py: 6100 keys over four ragged blocks."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile

    rng = np.random.default_rng(len("too_many"))
    n = 40_000
    val = rng.normal(0, 50, n).astype(np.float32)
    w = rng.integers(-500, 500, n).astype(np.int32)
    cuts = [0, 11_000, 11_001, 29_500, n]
    key = rng.integers(-100, 6000, n).astype(np.int32)
    path = tmp_path / "t.bin"
    BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("v", T.FLOAT), ("w", T.INTEGER)],
                                     [[key[lo:hi], val[lo:hi], w[lo:hi]] for lo, hi in zip(cuts, cuts[1:])])
    api = _api()
    return (api.DataFrame().table(str(path)).filter(api.Col("v") > -60.0).group_by(api.Col("k"))
            .agg(api.F.sum(api.Col("v") * 1.5).alias("s"), api.F.avg(api.Col("w")).alias("a"), api.F.count(),
                 api.F.min(api.Col("v")).alias("lo"), api.F.max(api.Col("w")).alias("hi")))


def test_the_refused_shape_runs_on_the_hbm_tier_and_stays_refused_by_default(tmp_path):
    from minispark_amd.hipspark import HipSparkError
    from minispark_amd.stage import NativeEngine, NativeStage, read_result_file
    from oracle.py_engine import run_query

    frame = _too_many(tmp_path)
    want = run_query(frame.task)
    assert len(want) > 4096
    with NativeEngine(0) as engine:
        stage = NativeStage(engine, frame.task, hbm_tier=True)
        try:
            for r in range(3):
                rows = stage.run()
                assert_rows_match(rows, want, max_ulps=0)
                stats = stage.stats()
                assert stats["tier"] == "hbm" and stats["partial_rows"] >= len(want) and stats["result_rows"] == len(want), stats
            assert stats["tier_switches"] == 2  # per-lane -> shared -> HBM, once: later runs start on the HBM tier
            out = stage.write(tmp_path / "result.bin")
            assert_rows_match(read_result_file(out), rows, max_ulps=0)
            # the several-rank entry points launch on buffers this tier has given up: refused, not run
            lib, flags, nrows = stage.lib, C.c_uint32(0), C.c_int64(0)
            assert lib.hs_stage_launch_partial(stage.handle, None) == 1 and lib.hs_stage_launch_finish(stage.handle, None, None, 1) == 1
            assert lib.hs_stage_wait(stage.handle, None, C.byref(flags), C.byref(nrows)) == 1 and lib.hs_stage_grow(stage.handle) == 1
            assert not lib.hs_stage_slab(stage.handle, None)
            assert stage.stats()["runs"] >= 3
        finally:
            stage.close()
        stage = NativeStage(engine, frame.task)
        try:
            with pytest.raises(HipSparkError, match="on-chip|LDS"):
                stage.run()
        finally:
            stage.close()


# ---- key kinds and shapes -------------------------------------------------------------------------------------------------
N_SHAPES = 300_000
CUTS = [0, 70_000, 70_001, 130_000, 150_000, 260_123, N_SHAPES]  # six ragged blocks; [130 000, 150 000) fails every WHERE


@pytest.fixture(scope="module")
def shapes_table(tmp_path_factory):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile, StrCol

    rng = np.random.default_rng(77)
    n = N_SHAPES
    alphabet = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", np.uint8)
    scode = rng.integers(0, 20_000, n)
    sbytes = np.stack([alphabet[(scode // 26**p) % 26] for p in range(4)], axis=1).astype(np.uint8)
    f = rng.normal(0, 100, n).astype(np.float32)
    f[130_000:150_000] = -1000.0 - rng.uniform(0, 10, 20_000).astype(np.float32)  # the block no WHERE keeps
    cols = {"k": rng.integers(-60_000, 60_000, n).astype(np.int32),
            "t": rng.integers(0, 100_000, n).astype(np.int64) * 86_400_000_000,
            "x": (rng.integers(0, 90_000, n) / 8.0).astype(np.float32),
            "s": StrCol(np.full(n, 4, np.uint8), sbytes.reshape(-1).copy()),
            "f": f, "g": rng.uniform(0, 1, n).astype(np.float32), "i": rng.integers(-1000, 1000, n).astype(np.int32)}
    schema = [("k", T.INTEGER), ("t", T.TIMESTAMP), ("x", T.FLOAT), ("s", T.STRING), ("f", T.FLOAT), ("g", T.FLOAT), ("i", T.INTEGER)]
    from minispark_amd.io import raw_slice

    path = tmp_path_factory.mktemp("hbm_shapes") / "t.bin"
    BlockFile(path).write_raw_blocks(schema, [[raw_slice(cols[name], lo, hi) for name, _ in schema] for lo, hi in zip(CUTS, CUTS[1:])])
    return path


def _aggregates(api, which):
    C_, F = api.Col, api.F
    return {"k": [F.sum(C_("f")).alias("a0"), F.count(), F.sum(C_("f") * (api.Lit(1) - C_("g"))).alias("a2"), F.max(C_("i")).alias("a3")],
            "t": [F.count()],  # no value column at all
            "x": [F.avg(C_("g")).alias("a0"), F.min(C_("f")).alias("a1"), F.sum(C_("i")).alias("a2")],
            "s": [F.sum(C_("i")).alias("a0"), F.avg(C_("i")).alias("a1"), F.count()],
            "computed": [F.min(C_("i")).alias("a0"), F.sum(C_("f")).alias("a1"), F.max(C_("g")).alias("a2")]}[which]


@pytest.mark.parametrize("where", ["none", "one", "nothing"])
@pytest.mark.parametrize("key", ["k", "t", "x", "s", "computed"])
def test_key_kinds_and_shapes(shapes_table, key, where):
    from minispark_amd.stage import NativeEngine, NativeStage
    from oracle.py_engine import run_query

    api = _api()
    df = api.DataFrame().table(str(shapes_table))
    if key == "computed":  # a SELECT in front: the key is an INTEGER expression the library materialises (hs_stage_plan.key_computed)
        df = df.select((api.Col("k") % 50_000 * 2 + api.Col("i") % 7).alias("kk"), api.Col("f"), api.Col("g"), api.Col("i"))
    if where == "one":
        df = df.filter(api.Col("f") > -500.0)
    elif where == "nothing":
        df = df.filter(api.Col("f") > 1.0e6)
    query = df.group_by(api.Col("kk" if key == "computed" else key)).agg(*_aggregates(api, key))
    want = run_query(query.task)
    assert (where == "nothing") == (want == [])
    with NativeEngine(0) as engine:
        stage = NativeStage(engine, query.task, hbm_tier=True)
        try:
            for _ in range(2):
                assert_rows_match(stage.run(), want, max_ulps=0)
            if want:
                assert len(want) > 4096 and stage.stats()["tier"] == "hbm"
        finally:
            stage.close()


def _random_query(tmp_path, seed):
    """The generator of test_random_scan_group_by_queries_through_the_stage_abi at sizes where the key ranges bite: 30 000 ..
    150 000 rows in one to five ragged blocks, INTEGER keys of up to 50 000 values, TIMESTAMP keys of up to 50 000 days, zero to
    two WHERE clauses (numeric, TIMESTAMP, STRING), one to five aggregates -> (query, its filters' names, the key column)."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.io import BlockFile, StrCol
    from minispark_amd.sql import Col, Functions as F, Lit

    rng, nr = random.Random(seed), np.random.default_rng(seed)
    n = rng.choice([30_000, 60_000, 100_000, 150_000])
    cols = {"k": nr.integers(-3, rng.choice([14, 5000, 20_000, 50_000]), n).astype(np.int32), "c": [rng.choice("ANR") for _ in range(n)],
            "f": nr.normal(0, 100, n).astype(np.float32), "g": nr.uniform(0, 1, n).astype(np.float32),
            "i": nr.integers(-1000, 1000, n).astype(np.int32),
            "t": (nr.integers(0, rng.choice([3000, 20_000, 50_000]), n).astype(np.int64) * 86_400_000_000)}
    schema = [("k", T.INTEGER), ("c", T.STRING), ("f", T.FLOAT), ("g", T.FLOAT), ("i", T.INTEGER), ("t", T.TIMESTAMP)]
    cuts = sorted({0, n, *[rng.randrange(0, n + 1) for _ in range(rng.choice([1, 2, 5]) - 1)]})
    path = tmp_path / "t.bin"
    BlockFile(path).write_raw_blocks(schema, [[cols["k"][lo:hi], StrCol.from_strings(cols["c"][lo:hi]), cols["f"][lo:hi],
                                               cols["g"][lo:hi], cols["i"][lo:hi], cols["t"][lo:hi]] for lo, hi in zip(cuts, cuts[1:])])
    df = DataFrame(object()).table(str(path))
    filters = {"g": Col("g") > 0.3, "i%3": Col("i") % 3 != 0, "f&g": (Col("f") < 50.0) & (Col("g") <= 0.9),
               "t": Col("t") <= "2010-01-01", "c": Col("c") != "N", "none_left": Col("i") > 5000}
    used = [rng.choice(sorted(filters)) for _ in range(rng.randint(0, 2))]
    for name in used:
        df = df.filter(filters[name])
    pool = [lambda: F.sum(Col("f")), lambda: F.sum(Col("i")), lambda: F.min(Col("f")), lambda: F.max(Col("i")),
            lambda: F.avg(Col("g")), lambda: F.sum(Col("f") * (Lit(1) - Col("g"))), lambda: F.min(Col("i")),
            lambda: F.max(Col("g")), lambda: F.avg(Col("i"))]
    aggs = [fn().alias(f"a{j}") for j, fn in enumerate(rng.sample(pool, rng.randint(1, 4)))]
    if rng.random() < 0.6:
        aggs.append(F.count())
    key = rng.choice(["k", "t", "k", "t", "k", "c"])
    return df.group_by(Col(key)).agg(*aggs), used, key


# what the generator draws for these seeds (replayed on the CPU against the oracle): seed -> the query has more than 4096 groups
# and therefore must end on the HBM tier
RANDOM_SEEDS = {0: True, 1: False, 4: True, 6: True, 7: True, 10: False, 11: True, 13: True}


@pytest.mark.parametrize("seed", sorted(RANDOM_SEEDS))
def test_random_scan_group_by_queries_on_the_hbm_tier(tmp_path, seed):
    """Random queries with hbm_tier=True: no refusal is accepted, every result equals the oracle's at 0 ulp, and the seeds with
    more than 4096 groups - most of them, a STRING filter and two stacked filters among them - run on the HBM tier."""
    from minispark_amd.stage import NativeEngine, NativeStage
    from oracle.py_engine import run_query

    query, used, key = _random_query(tmp_path, seed)
    want = run_query(query.task)
    assert (len(want) > 4096) == RANDOM_SEEDS[seed], (seed, key, used, len(want))
    with NativeEngine(0) as engine:
        stage = NativeStage(engine, query.task, hbm_tier=True)
        try:
            for _ in range(3):
                assert_rows_match(stage.run(), want, max_ulps=0)
                if len(want) > 4096:
                    assert stage.stats()["tier"] == "hbm", (seed, key, used, stage.stats())
        finally:
            stage.close()


def test_the_random_seeds_reach_the_hbm_tier_with_string_and_stacked_filters(tmp_path):
    """Host only in effect (no stage is run): the seeds above are not a hollow set."""
    drawn = {}
    for seed in RANDOM_SEEDS:
        if RANDOM_SEEDS[seed]:
            (tmp_path / str(seed)).mkdir()
            drawn[seed] = _random_query(tmp_path / str(seed), seed)[1:]
    assert len(drawn) >= 5
    assert any("c" in used for used, _ in drawn.values()) and any(len(used) == 2 for used, _ in drawn.values())
    assert {key for _, key in drawn.values()} == {"k", "t"}


def test_data_errors_surface_for_surviving_rows_only(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile
    from minispark_amd.stage import NativeEngine, NativeStage

    rng = np.random.default_rng(5)
    n = 50_000
    k = rng.permutation(n).astype(np.int32)
    f = rng.normal(0, 10, n).astype(np.float32)
    i = rng.integers(1, 100, n).astype(np.int32)
    big = np.full(n, 2_000_000_000, np.int32)
    half = np.concatenate([np.arange(n // 2), np.arange(n // 2)]).astype(np.int32)  # every key twice inside the one block
    path = tmp_path / "t.bin"
    BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("f", T.FLOAT), ("i", T.INTEGER), ("big", T.INTEGER), ("h", T.INTEGER)],
                                     [[k, f, i, big, half]])
    api = _api()
    Col, F = api.Col, api.F
    def table():  # (a frame's builder calls extend the frame itself: a fresh one per query)
        return api.DataFrame().table(str(path))

    with NativeEngine(0) as engine:
        def run(query):
            stage = NativeStage(engine, query.task, hbm_tier=True)
            try:
                return stage.run()
            finally:
                stage.close()

        with pytest.raises(ZeroDivisionError):
            run(table().group_by(Col("k")).agg(F.sum(Col("f") / (Col("i") - Col("i"))).alias("s")))
        # the same argument behind a WHERE that drops every offending row (all of them: nothing is left to raise)
        assert run(table().filter(Col("i") < 0).group_by(Col("k")).agg(F.sum(Col("f") / (Col("i") - Col("i"))).alias("s"))) == []
        # ... and with survivors whose divisor is not zero
        rows = run(table().filter(Col("i") > 50).group_by(Col("k")).agg(F.sum(Col("f") / (Col("i") - 50)).alias("s")))
        assert len(rows) == int((i > 50).sum())
        with pytest.raises(OverflowError):  # 2e9 + 2e9 inside one block: the partial row does not fit the shuffle file's i32
            run(table().group_by(Col("h")).agg(F.sum(Col("big")).alias("s")))


def test_a_result_larger_than_one_block(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import BlockFile
    from minispark_amd.stage import NativeEngine, NativeStage

    rng = np.random.default_rng(9)
    n = 3_000_000
    k = rng.integers(0, 9_000_000, n).astype(np.int32)
    i = rng.integers(-1000, 1000, n).astype(np.int32)
    cuts = [0, 1_000_000, 1_900_000, n]
    path = tmp_path / "t.bin"
    BlockFile(path).write_raw_blocks([("k", T.INTEGER), ("i", T.INTEGER)], [[k[lo:hi], i[lo:hi]] for lo, hi in zip(cuts, cuts[1:])])
    api = _api()
    query = api.DataFrame().table(str(path)).group_by(api.Col("k")).agg(api.F.count(), api.F.sum(api.Col("i")).alias("s"))
    keys, inverse, counts = np.unique(k, return_inverse=True, return_counts=True)
    sums = np.zeros(len(keys), np.int64)
    np.add.at(sums, inverse, i)
    assert len(keys) > 2 * 1024 * 1024
    with NativeEngine(0) as engine:
        stage = NativeStage(engine, query.task, hbm_tier=True)
        try:
            stage.run()
            names = [name for name, _ in stage.schema]
            raw = dict(zip(names, stage.raw_columns()))
            order = np.argsort(raw["k"], kind="stable")
            assert np.array_equal(raw["k"][order], keys)
            count_name = next(nm for nm in names if nm not in ("k", "s"))
            assert np.array_equal(raw[count_name][order], counts) and np.array_equal(raw["s"][order], sums)
            out = stage.write(tmp_path / "result.bin")
            f = BlockFile(out)
            assert len(f.block_starts) == 2
            blocks = [f.read_block_raw(b) for b in range(2)]
            for c, name in enumerate(names):
                assert np.array_equal(np.concatenate([blk[c] for blk in blocks]), raw[name]), name
        finally:
            stage.close()


# ---- the kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_filters", [0, 1, 2])
def test_hs_agg_rows_against_numpy(n_filters):
    import torch

    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.sql import Col, Functions as F, Lit

    lib = hs.load_library()
    rng = np.random.default_rng(n_filters)
    n = 100_003
    k = rng.integers(0, 1000, n).astype(np.int32)
    f = rng.normal(0, 10, n).astype(np.float32)
    i = rng.integers(-5, 5, n).astype(np.int32)
    schema = [("k", T.INTEGER), ("f", T.FLOAT), ("i", T.INTEGER)]
    kinds = [hs.I32, hs.F32, hs.I32]
    filters = [Col("i") != 0, Col("f") > -5.0][:n_filters]
    # literal (COUNT), bare FLOAT column, bare INTEGER column, a computed FLOAT cell that divides by zero where i == 0
    aggs = [F.count(), F.sum(Col("f")).alias("a"), F.max(Col("i")).alias("b"), F.sum(Col("f") / Col("i")).alias("c")]
    low = lower_aggregate(schema, kinds, filters, Col("k"), aggs)
    host = {"k": k, "f": f, "i": i}
    dev = {name: torch.from_numpy(a).cuda() for name, a in host.items()}
    names = [schema[idx][0] for idx in low.program.columns]
    cols = (hs.hs_col * len(names))(*[hs.hs_col(kinds[[s for s, _ in schema].index(nm)], -1, dev[nm].data_ptr(), None, None) for nm in names])
    prog, spec = low.program.to_struct(), low.spec()
    na = spec.n_acc
    vk, vs, cc, nfil = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_uint64 * 16)(), C.c_int32(0)
    hs.check(lib.hs_agg_rows_classify(cols, len(names), low.key_slot, C.byref(prog), C.byref(spec), vk, vs, cc, C.byref(nfil)))
    assert nfil.value == n_filters
    got_kinds = sorted(int(vk[a]) for a in range(na))
    assert got_kinds == sorted([-1, hs.F32, hs.I32, hs.F64])
    units = np.array([0, 1, 1, 50_000, 50_001, n], np.int64)  # a 1-row unit, an empty unit, ragged boundaries
    n_units = len(units) - 1
    d_units = torch.from_numpy(units).cuda()
    out_key = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    outs = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(na)]  # 8 bytes per row: room for any kind
    ptrs = (C.c_void_p * 16)(*[o.data_ptr() for o in outs])
    bounds = torch.zeros(n_units + 1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(lib.hs_agg_rows_ws_bytes(n, n_units) // 8 + 2, dtype=torch.int64, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    hs.check(lib.hs_agg_rows(None, cols, len(names), low.key_slot, C.byref(prog), C.byref(spec), d_units.data_ptr(), n_units, n,
                             out_key.data_ptr(), ptrs, vk, bounds.data_ptr(), ws.data_ptr(), flags.data_ptr()), "hs_agg_rows")
    torch.cuda.synchronize()
    keep = np.ones(n, bool)
    if n_filters >= 1:
        keep &= i != 0
    if n_filters >= 2:
        keep &= f > -5.0
    rows = np.flatnonzero(keep)
    want_bounds = np.searchsorted(rows, units, side="left")
    assert np.array_equal(bounds.cpu().numpy(), want_bounds)
    m = len(rows)
    assert np.array_equal(out_key.cpu().numpy()[:m], k[rows])  # positions are exactly the surviving rows, in order
    assert (out_key.cpu().numpy()[m:] == -7).all()
    for a in range(na):
        kind = int(vk[a])
        raw = outs[a].cpu().numpy()
        if kind == -1:
            assert cc[a] == 1 and not raw.any()
        elif kind == hs.F32:
            assert np.array_equal(raw.view(np.float32)[:m].view(np.uint32), f[rows].view(np.uint32))
        elif kind == hs.I32:
            assert np.array_equal(raw.view(np.int32)[:m], i[rows])
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                cell = f[rows].astype(np.float64) / i[rows].astype(np.float64)
            ok = i[rows] != 0
            assert np.array_equal(raw.view(np.float64)[:m][ok].view(np.uint64), cell[ok].view(np.uint64))
    # the division by zero is raised by surviving rows only: the first filter drops every row with i == 0
    assert bool(int(flags.cpu()[0]) & hs.FLAG_DIV_ZERO) == (n_filters == 0)


def test_hs_agg_rows_copies_string_keys_of_other_fixed_lengths():
    """A fixed-length STRING key that is not 1 / 2 / 4 bytes wide (the stages refuse or recode those; the radix tier takes up to
    16 bytes) is copied byte by byte from where it lies."""
    import torch

    from minispark_amd import hipspark as hs
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.sql import Col, Functions as F

    lib = hs.load_library()
    rng = np.random.default_rng(3)
    n = 20_001
    key = rng.integers(65, 91, (n, 3)).astype(np.uint8)
    i = rng.integers(-5, 5, n).astype(np.int32)
    schema, kinds = [("s", T.STRING), ("i", T.INTEGER)], [hs.STR, hs.I32]
    low = lower_aggregate(schema, kinds, [Col("i") > 0], Col("s"), [F.sum(Col("i")).alias("a")])
    d_key, d_i, d_lens = torch.from_numpy(key.reshape(-1).copy()).cuda(), torch.from_numpy(i).cuda(), torch.full((n,), 3, dtype=torch.uint8).cuda()
    by_name = {"s": hs.hs_col(hs.STR, 3, d_key.data_ptr(), d_lens.data_ptr(), None), "i": hs.hs_col(hs.I32, -1, d_i.data_ptr(), None, None)}
    names = [schema[idx][0] for idx in low.program.columns]
    cols = (hs.hs_col * len(names))(*[by_name[nm] for nm in names])
    prog, spec = low.program.to_struct(), low.spec()
    units = np.array([0, 7_000, n], np.int64)
    d_units = torch.from_numpy(units).cuda()
    out_key = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    out_val = torch.zeros(n, dtype=torch.int32, device="cuda")
    ptrs, vk = (C.c_void_p * 16)(out_val.data_ptr()), (C.c_int32 * 16)(hs.I32)
    bounds = torch.zeros(3, dtype=torch.int64, device="cuda")
    ws = torch.zeros(lib.hs_agg_rows_ws_bytes(n, 2) // 8 + 2, dtype=torch.int64, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    hs.check(lib.hs_agg_rows(None, cols, len(names), low.key_slot, C.byref(prog), C.byref(spec), d_units.data_ptr(), 2, n,
                             out_key.data_ptr(), ptrs, vk, bounds.data_ptr(), ws.data_ptr(), flags.data_ptr()), "hs_agg_rows")
    torch.cuda.synchronize()
    rows = np.flatnonzero(i > 0)
    m = len(rows)
    assert np.array_equal(bounds.cpu().numpy(), np.searchsorted(rows, units))
    got = out_key.cpu().numpy().reshape(n, 3)
    assert np.array_equal(got[:m], key[rows]) and not got[m:].any()
    assert np.array_equal(out_val.cpu().numpy()[:m], i[rows]) and int(flags.cpu()[0]) == 0
