"""The JOIN-to-rows stage behind the C ABI (hs_join_select_stage_*, minispark_amd/stage.py NativeJoinSelectStage): the golden
join queries through the library alone - as a row multiset against the reference's goldens and in exact order against
HipExecutionEngine - and generated multi-block tables in exact order against a numpy model of the engine's order (JoinJob
= hash(key) % 10, probe row, build row), on every route: dense, hashed, hashed-string and the global table."""

from __future__ import annotations

import numpy as np
import pytest

from tests.conftest import assert_rows_match, load_golden
from tests.queries import case_by_name
from tests.test_gpu_join_str_windows import fnv1a, model_pairs, overflow_keys

pytestmark = pytest.mark.gpu

GOLDENS = ["e2e_join_select", "e2e_join_where_float", "e2e_join_where_ts", "fruits5_self_join"]


def _api(engine):
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    return api_namespace(lambda: DataFrame(engine), Col, Functions, Lit)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_joins_through_the_c_abi(tmp_path, name):
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.stage import NativeEngine, NativeJoinSelectStage, read_result_file

    golden = load_golden(name)
    case = case_by_name(name)
    with HipExecutionEngine(device=0) as eng:
        want = case.build(_api(eng), golden["paths"]).collect()
    with NativeEngine(0) as engine:
        stage = NativeJoinSelectStage(engine, case.build(_api(object()), golden["paths"]).task)
        first = stage.run(tmp_path / "a.bin")
        assert first == read_result_file(tmp_path / "a.bin")
        second = stage.run(tmp_path / "b.bin")
        stats = stage.stats()
        stage.close()
    assert_rows_match(first, golden["rows"])
    assert first == want  # the engine's order, exactly
    assert second == first
    assert stats["runs"] == 2 and stats["rows"] == len(first)
    assert stats["route"] == ("hashed-string" if name == "fruits5_self_join" else "dense")


def _str_col(values: list[bytes]):
    from minispark_amd.io import StrCol

    lens = np.array([len(v) for v in values], np.uint8)
    return StrCol(lens, np.frombuffer(b"".join(values), np.uint8).copy())


def _write(path, schema, cols, block_rows):
    from minispark_amd.io import BlockFile, raw_slice

    n = len(cols[0])
    blocks = [[raw_slice(c, lo, min(lo + block_rows, n)) for c in cols] for lo in range(0, n, block_rows)]
    BlockFile(path).write_raw_blocks(schema, blocks)


def _read_raw(path):
    from minispark_amd.io import BlockFile, raw_concat

    f = BlockFile(path)
    blocks = [f.read_block_raw(b) for b in range(len(f.block_starts))]
    return [raw_concat([blk[c] for blk in blocks]) for c in range(len(blocks[0]))]


def _part_int(keys: np.ndarray) -> np.ndarray:
    h = keys.astype(np.int64)
    h[h == -1] = -2  # hash(-1) == -2 in CPython
    return np.mod(h, 10)


def _run_generated(tmp_path, bkeys, pkeys, bcodes, pcodes, bparts, pparts, route, block_rows=1 << 20):
    """Tables (key, row id) on both sides -> the stage -> (brow, prow) of every result row checked against the model."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.stage import NativeEngine, NativeJoinSelectStage

    kt = T.STRING if isinstance(bkeys, list) else T.INTEGER
    nb, np_ = len(bcodes), len(pcodes)
    _write(tmp_path / "b.bin", [("bk", kt), ("brow", T.INTEGER)],
           [_str_col(bkeys) if kt == T.STRING else bkeys.astype(np.int32), np.arange(nb, dtype=np.int32)], block_rows)
    _write(tmp_path / "p.bin", [("pk", kt), ("prow", T.INTEGER)],
           [_str_col(pkeys) if kt == T.STRING else pkeys.astype(np.int32), np.arange(np_, dtype=np.int32)], block_rows)
    api = _api(object())
    C_ = api.Col
    q = api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                             on=C_("bk") == C_("pk"), how="inner")
    with NativeEngine(0) as engine:
        stage = NativeJoinSelectStage(engine, q.task)
        n = stage.run_to_file(tmp_path / "out.bin", rows_per_block=1 << 20)
        stats = stage.stats()
        stage.close()
    porder = np.argsort(pparts, kind="stable")
    left, right = model_pairs(bcodes, pcodes[porder])
    assert n == len(left) and stats["route"] == route
    out = _read_raw(tmp_path / "out.bin")
    assert np.array_equal(out[1], left.astype(np.int32))
    assert np.array_equal(out[3], porder[right].astype(np.int32))
    if kt == T.INTEGER:
        assert np.array_equal(out[0], bkeys[left].astype(np.int32)) and np.array_equal(out[0], out[2])
    else:
        assert np.array_equal(out[0].lens, out[2].lens) and np.array_equal(out[0].data, out[2].data)
        head = left[:2000]
        assert out[0].lens[: len(head)].tolist() == [len(bkeys[i]) for i in head]
        assert out[0].data[: sum(len(bkeys[i]) for i in head)].tobytes() == b"".join(bkeys[i] for i in head)


@pytest.mark.parametrize("shape", ["dense", "sparse", "large"])
def test_generated_integer_joins_in_the_engines_order(tmp_path, shape):
    rng = np.random.default_rng(5)
    if shape == "dense":  # 0 .. 40 000 with duplicates on both sides
        nb, np_ = 60_000, 150_000
        bkeys, pkeys = rng.integers(-20, 40_000, nb), rng.integers(-50, 41_000, np_)
        route = "dense"
    elif shape == "sparse":  # a sparse range with negative keys and -1
        nb, np_ = 80_000, 200_000
        pool = np.concatenate([rng.integers(-(2**31) + 1, 2**31 - 1, 40_000), [-1, -2, 0, 1]])
        bkeys, pkeys = pool[rng.integers(0, len(pool), nb)], pool[rng.integers(0, len(pool), np_)]
        route = "hashed"
    else:  # 3 M build x 12 M probe rows, a sparse range: many hash windows
        nb, np_ = 3_000_000, 12_000_000
        pool = rng.integers(-(2**30), 2**30, 2_500_000) * 2 + 1
        bkeys, pkeys = pool[rng.integers(0, len(pool), nb)], rng.integers(-(2**30), 2**30, np_) * 2 + 1
        pkeys[::3] = pool[rng.integers(0, len(pool), len(pkeys[::3]))]
        route = "hashed"
    _run_generated(tmp_path, bkeys, pkeys, bkeys, pkeys, _part_int(bkeys), _part_int(pkeys), route,
                   block_rows=1 << 20 if shape == "large" else 17_000)


def _str_keys(rng, n_distinct: int):
    base = [bytes(rng.integers(97, 123, int(rng.integers(0, 41))).astype(np.uint8)) for _ in range(n_distinct)]
    base += [b"", b"z" * 40, b"z" * 39 + b"y"]
    base += [b[:-1] + bytes([b[-1] ^ 1]) for b in base[:200] if len(b) > 0]  # keys differing only in their last byte
    return list(dict.fromkeys(base))


def _codes_and_parts(keys: list[bytes], code: dict, miss0: int = 0):
    codes = np.array([code.get(k, -1 - miss0 - i) for i, k in enumerate(keys)], np.int64)
    width = max(len(k) for k in keys) if keys else 1
    mat = np.zeros((len(keys), max(width, 1)), np.uint8)
    lens = np.array([len(k) for k in keys], np.int64)
    flat = np.frombuffer(b"".join(keys), np.uint8)
    rows = np.repeat(np.arange(len(keys)), lens)
    cols = np.arange(len(flat)) - np.repeat(np.cumsum(lens) - lens, lens)
    mat[rows, cols] = flat
    parts = (fnv1a(mat, lens) % np.uint64(10)).astype(np.int64)
    return codes, parts


@pytest.mark.parametrize("size", ["small", "large"])
def test_generated_string_joins_in_the_engines_order(tmp_path, size):
    rng = np.random.default_rng(11)
    nd, nb, np_ = (3_000, 20_000, 50_000) if size == "small" else (1_500_000, 3_000_000, 12_000_000)
    base = _str_keys(rng, nd)
    code = {k: i for i, k in enumerate(base)}
    bkeys = [base[i] for i in rng.integers(0, len(base), nb)]
    pidx = rng.integers(0, len(base) + len(base) // 4, np_)
    pkeys = [base[i] if i < len(base) else b"miss%d" % i for i in pidx]
    bcodes, bparts = _codes_and_parts(bkeys, code)
    pcodes, pparts = _codes_and_parts(pkeys, code, miss0=10)
    _run_generated(tmp_path, bkeys, pkeys, bcodes, pcodes, bparts, pparts, "hashed-string",
                   block_rows=1 << 20 if size == "large" else 7_000)


def test_an_overflowing_window_takes_the_global_table(tmp_path):
    keys = overflow_keys()
    code = {k: i for i, k in enumerate(keys)}
    probe = keys[::-1] + keys[:50] + [b"absent"]
    bcodes, bparts = _codes_and_parts(keys, code)
    pcodes, pparts = _codes_and_parts(probe, code, miss0=10)
    _run_generated(tmp_path, keys, probe, bcodes, pcodes, bparts, pparts, "global", block_rows=256)


def test_refusals_need_no_gpu_work(tmp_path):
    from minispark_amd.stage import StageUnsupported, lower_join_select_stage_plan

    g = load_golden("e2e_join_select")
    api = _api(object())
    C_, F = api.Col, api.F

    def joined(on=None):
        u = api.DataFrame().table(g["paths"]["users"]).alias("u")
        o = api.DataFrame().table(g["paths"]["orders"]).alias("o")
        return u.join(o, on=on if on is not None else C_("u.user_id") == C_("o.user_id"), how="inner")

    with pytest.raises(StageUnsupported):
        lower_join_select_stage_plan(joined().group_by(C_("u.country")).agg(F.count().alias("n")).task)
    with pytest.raises(StageUnsupported):
        lower_join_select_stage_plan(joined(C_("u.user_id") == C_("o.product")).task)
    with pytest.raises(StageUnsupported):
        lower_join_select_stage_plan(joined().filter(C_("u.age") > C_("o.quantity")).select(C_("u.first_name")).task)
