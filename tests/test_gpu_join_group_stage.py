"""The general join feeding a GROUP BY behind the C ABI (hs_join_group_stage_*, minispark_amd/stage.py NativeJoinGroupStage):
the golden join aggregates and the dictionary-join queries with duplicate build keys through the library alone, STRING join
keys, a WHERE over both sides, GROUP BY keys of either side and kind, every join route, capacity growth and its limit, empty
results, generated multi-block tables against HipExecutionEngine, and the gathered aggregate without the run-time compiler
against the pair-indexed one."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, assert_rows_match, load_golden
from tests.queries import case_by_name
from tests.test_gpu_join_dict import _join_queries, _join_tables, _oracle_api
from tests.test_gpu_join_select_stage import _codes_and_parts, _str_col, _write
from tests.test_gpu_join_str_windows import overflow_keys

pytestmark = pytest.mark.gpu


def _api():
    return _oracle_api()


def _run_stage(tmp_path, task, runs=3, n_parts=None):
    """The stage on `task`, `runs` times -> (rows of every run, stats after the last)."""
    from minispark_amd.stage import NativeEngine, NativeJoinGroupStage

    out = []
    with NativeEngine(0) as engine:
        stage = NativeJoinGroupStage(engine, task, n_parts=n_parts)
        try:
            for r in range(runs):
                path = tmp_path / f"run{r}.bin"
                rows = stage.run(path)  # (read back from the result file the library wrote: no file for no rows)
                assert path.exists() == bool(rows)
                out.append(rows)
            stats = stage.stats()
        finally:
            stage.close()
    return out, stats


def _check(runs, want):
    for rows in runs:
        assert assert_rows_match(rows, want, max_ulps=1) <= 2


def _oracle(task):
    from oracle.py_engine import run_query

    return run_query(task)


@pytest.mark.parametrize("name", ["join_group", "e2e_join_group_count", "e2e_join_group_sum"])
def test_golden_join_aggregates_through_the_c_abi(tmp_path, name):
    golden = load_golden(name)
    runs, stats = _run_stage(tmp_path, case_by_name(name).build(_api(), golden["paths"]).task)
    _check(runs, golden["rows"])
    assert stats["runs"] == 3 and stats["aggregate"] == "pairs"  # numeric arguments read through the pair rows
    assert stats["dictionary"] > 0  # every one of them groups by a variable-length STRING


def test_having_after_the_join_is_refused():
    from minispark_amd.stage import StageUnsupported, lower_join_group_stage_plan

    golden = load_golden("e2e_join_group_having")
    with pytest.raises(StageUnsupported, match="HAVING"):
        lower_join_group_stage_plan(case_by_name("e2e_join_group_having").build(_api(), golden["paths"]).task)


@pytest.mark.parametrize("name", ["config4", "filtered_with_build_side_argument", "probe_side_int_key",
                                  "filtered_on_the_probe_side", "count_only"])
def test_dictionary_join_queries_with_a_key_twice(tmp_path, name):
    orders, lineitem = _join_tables(tmp_path, 3000 if name != "probe_side_int_key" else 300, 20_000, seed=21, dup=True)
    task = _join_queries(_api(), orders, lineitem)[name].task
    runs, stats = _run_stage(tmp_path, task)
    _check(runs, _oracle(task))
    assert stats["route"] == "dense" and stats["pairs"] > 0 and stats["aggregate"] == "pairs"


def _mixed_tables(tmp_path, nb=4000, np_=30_000, seed=3, block_rows=3000):
    """b(bk INT with duplicates, bs STRING 5 values, bi INT, bt STRING key) x p(pk INT, pf FLOAT, pts TIMESTAMP, ps STRING
    4 values, pi INT, pt STRING key)."""
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(seed)
    names = [b"alpha", b"be", b"gamma-ray", b"d", b"epsilon"]
    colours = [b"red", b"green", b"blue-ish", b"violet"]
    skeys = [b"k%d" % i for i in range(1500)]
    bk = rng.integers(0, 2000, nb)
    _write(tmp_path / "b.bin", [("bk", T.INTEGER), ("bs", T.STRING), ("bi", T.INTEGER), ("bt", T.STRING)],
           [bk.astype(np.int32), _str_col([names[i] for i in rng.integers(0, 5, nb)]), rng.integers(-5, 6, nb).astype(np.int32),
            _str_col([skeys[i] for i in rng.integers(0, 1500, nb)])], block_rows)
    ts0 = 1_700_000_000_000_000
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("pf", T.FLOAT), ("pts", T.TIMESTAMP), ("ps", T.STRING), ("pi", T.INTEGER),
                                ("pt", T.STRING)],
           [rng.integers(-100, 2100, np_).astype(np.int32), np.round(rng.uniform(0, 100, np_), 2).astype(np.float32),
            (ts0 + rng.integers(0, 7, np_) * 86_400_000_000).astype(np.int64),
            _str_col([colours[i] for i in rng.integers(0, 4, np_)]), rng.integers(0, 300, np_).astype(np.int32),
            _str_col([skeys[i] if i < 1500 else b"none" for i in rng.integers(0, 1700, np_)])], block_rows)
    return str(tmp_path / "b.bin"), str(tmp_path / "p.bin")


def _mixed_query(api, b, p, kind):
    C, F = api.Col, api.F
    bt, pt = api.DataFrame().table(b), api.DataFrame().table(p)
    if kind == "string_keys":
        j = bt.join(pt, on=C("bt") == C("pt"), how="inner")
        # (JoinJobs of STRING keys hash differently from the oracle's: f32 partial sums would round apart, exact ones cannot)
        return j.group_by(C("bs")).agg(F.sum(C("pi") * C("bi")).alias("w"), F.max(C("pf")).alias("m"), F.count())
    j = bt.join(pt, on=C("bk") == C("pk"), how="inner")
    if kind == "cross_side_where":
        return j.filter((C("pf") > C("bi") * 10) & (C("pi") < 250)).group_by(C("bs")).agg(F.sum(C("pf")).alias("s"), F.count())
    if kind == "build_int_key":
        return j.group_by(C("bi")).agg(F.sum(C("pf")).alias("s"), F.max(C("pi")).alias("m"), F.count())
    if kind == "probe_timestamp_key":
        return j.group_by(C("pts")).agg(F.min(C("pf")).alias("lo"), F.count())
    if kind == "probe_string_key":
        return j.filter(C("bs") != "d").group_by(C("ps")).agg(F.avg(C("pf")).alias("a"), F.count())
    if kind == "growth":
        return j.group_by(C("pi")).agg(F.sum(C("pf")).alias("s"), F.count())
    if kind == "empty_where":
        return j.filter(C("pf") > 1000.0).group_by(C("bs")).agg(F.count())
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["string_keys", "cross_side_where", "build_int_key", "probe_timestamp_key", "probe_string_key",
                                  "growth", "empty_where"])
def test_generated_join_aggregates_match_the_oracle(tmp_path, kind):
    b, p = _mixed_tables(tmp_path)
    task = _mixed_query(_api(), b, p, kind).task
    runs, stats = _run_stage(tmp_path, task)
    want = _oracle(task)
    _check(runs, want)
    if kind == "string_keys":
        assert stats["route"] == "hashed-string"
    elif kind != "empty_where":  # (no probe row survives: nothing is joined)
        assert stats["route"] == "dense"
    if kind == "growth":
        assert stats["grows"] >= 1 and len(want) == 300
    if kind == "empty_where":
        assert want == [] and stats["probe_rows"] == 0
    if kind == "probe_string_key":
        assert stats["dictionary"] == 4


def test_an_empty_join(tmp_path):
    from minispark_amd.constants import ColumnType as T

    _write(tmp_path / "b.bin", [("bk", T.INTEGER), ("bs", T.STRING)], [np.arange(100, dtype=np.int32), _str_col([b"x"] * 100)], 50)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("pf", T.FLOAT)], [np.arange(1000, 1400, dtype=np.int32),
                                                                      np.ones(400, np.float32)], 128)
    api = _api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                 on=C("bk") == C("pk"), how="inner")
            .group_by(C("bs")).agg(F.sum(C("pf")).alias("s"))).task
    runs, stats = _run_stage(tmp_path, task)
    assert runs == [[], [], []] and stats["pairs"] == 0 and _oracle(task) == []


@pytest.mark.parametrize("route", ["hashed", "global"])
def test_join_routes_through_stats(tmp_path, route):
    from minispark_amd.constants import ColumnType as T

    rng = np.random.default_rng(8)
    if route == "hashed":  # a sparse key range
        pool = rng.integers(-(2**31) + 1, 2**31 - 1, 3000)
        bk, pk = pool[rng.integers(0, 3000, 5000)], pool[rng.integers(0, 3000, 20_000)]
        bcol, pcol, kt = bk.astype(np.int32), pk.astype(np.int32), T.INTEGER
        n_b, n_p = len(bk), len(pk)
    else:  # more STRING keys in one LDS window than it holds
        keys = overflow_keys()
        probe = keys[::-1] + keys[:50] + [b"absent"]
        bcol, pcol, kt = _str_col(keys), _str_col(probe), T.STRING
        n_b, n_p = len(keys), len(probe)
    _write(tmp_path / "b.bin", [("bk", kt), ("g", T.INTEGER)], [bcol, rng.integers(0, 7, n_b).astype(np.int32)], 256)
    _write(tmp_path / "p.bin", [("pk", kt), ("v", T.FLOAT)], [pcol, np.round(rng.uniform(0, 9, n_p), 1).astype(np.float32)], 1000)
    api = _api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                 on=C("bk") == C("pk"), how="inner")
            .group_by(C("g")).agg(F.sum(C("v")).alias("s"), F.count())).task
    runs, stats = _run_stage(tmp_path, task)
    _check(runs, _oracle(task))
    assert stats["route"] == route


def test_too_many_groups_is_refused_as_on_chip(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.hipspark import HipSparkError

    n = 300_000
    _write(tmp_path / "b.bin", [("bk", T.INTEGER)], [np.arange(1000, dtype=np.int32)], 500)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("g", T.INTEGER)],
           [(np.arange(n) % 1000).astype(np.int32), np.arange(n, dtype=np.int32)], 1 << 16)
    api = _api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                 on=C("bk") == C("pk"), how="inner")
            .group_by(C("g")).agg(F.count())).task
    with pytest.raises(HipSparkError, match="on-chip"):
        _run_stage(tmp_path, task, runs=1)


def test_generated_3m_by_12m_rows_match_the_engine(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    rng = np.random.default_rng(12)
    nb, np_ = 3_000_000, 12_000_000
    pool = rng.integers(-(2**30), 2**30, 2_000_000) * 2 + 1
    bk = pool[rng.integers(0, len(pool), nb)].astype(np.int32)
    pk = pool[rng.integers(0, len(pool), np_)].astype(np.int32)
    _write(tmp_path / "b.bin", [("bk", T.INTEGER), ("bs", T.STRING), ("bi", T.INTEGER)],
           [bk, _str_col([(b"g%d" % i) for i in rng.integers(0, 5, nb)]), rng.integers(1, 4, nb).astype(np.int32)], 1 << 20)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("pf", T.FLOAT)], [pk, rng.integers(1, 100, np_).astype(np.float32)], 1 << 20)

    def query(api):
        C, F = api.Col, api.F
        return (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                     on=C("bk") == C("pk"), how="inner")
                .group_by(C("bs")).agg(F.sum(C("pf") * C("bi")).alias("w"), F.count()))

    with HipExecutionEngine(device=0) as eng:
        want = query(engine_api(eng)).collect()
    runs, stats = _run_stage(tmp_path, query(_api()).task)
    _check(runs, want)
    assert stats["route"] == "hashed" and stats["pairs"] > np_ // 2


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from minispark_amd import hipspark as hs
from minispark_amd.stage import NativeEngine, NativeJoinGroupStage
from tests.conftest import load_golden
from tests.queries import case_by_name
from tests.test_gpu_join_dict import _oracle_api
golden = load_golden("join_group")
with NativeEngine(0) as engine:
    stage = NativeJoinGroupStage(engine, case_by_name("join_group").build(_oracle_api(), golden["paths"]).task)
    rows = stage.run(sys.argv[2])
    stats = stage.stats()
    stage.close()
import ctypes
counters = (ctypes.c_int32 * 3)()
hs.load_library().hs_jit_stats(counters)
print(json.dumps({"rows": rows, "aggregate": stats["aggregate"], "jit_launches": counters[1]}, default=str))
"""


def test_the_gathered_route_without_the_jit_in_a_child_process(tmp_path):
    golden = load_golden("join_group")
    env = dict(os.environ, HIPSPARK_JIT="0")
    proc = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(tmp_path / "child.bin")], env=env, capture_output=True,
                          text=True, timeout=600, cwd=str(ROOT))
    assert proc.returncode == 0, proc.stderr[-2000:]
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert got["aggregate"] == "gathered" and got["jit_launches"] == 0
    runs, _ = _run_stage(tmp_path, case_by_name("join_group").build(_api(), golden["paths"]).task, runs=1)
    assert assert_rows_match(got["rows"], golden["rows"], max_ulps=1) <= 2
    assert assert_rows_match(got["rows"], runs[0], max_ulps=1) <= 2  # the pair-indexed route in this process
