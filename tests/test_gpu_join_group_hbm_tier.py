"""The HBM (radix) aggregation tier behind the join feeding a GROUP BY (hs_join_group_stage_set_hbm_tier,
NativeJoinGroupStage(hbm_tier=True)): the JoinJobs' pair ranges are the units, the columns are gathered through the pair rows,
the tail is the scan stage's - against the Python oracle at 0 ulp."""

from __future__ import annotations

import numpy as np
import pytest

from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu


def _oracle_api():
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    return api_namespace(lambda: DataFrame(object()), Col, Functions, Lit)


def _write(path, schema, cols, block_rows):
    from minispark_amd.io import BlockFile, raw_slice

    n = len(cols[0])
    BlockFile(path).write_raw_blocks(schema, [[raw_slice(c, lo, min(lo + block_rows, n)) for c in cols] for lo in range(0, n, block_rows)])


def _run(tmp_path, task, hbm_tier, runs=2, n_parts=None):
    from minispark_amd.stage import NativeEngine, NativeJoinGroupStage

    out = []
    with NativeEngine(0) as engine:
        stage = NativeJoinGroupStage(engine, task, hbm_tier=hbm_tier, n_parts=n_parts)
        try:
            for r in range(runs):
                out.append(stage.run(tmp_path / f"run{r}.bin"))
            stats = stage.stats()
        finally:
            stage.close()
    return out, stats


def test_too_many_groups_run_on_the_hbm_tier_and_stay_refused_by_default(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.hipspark import HipSparkError
    from oracle.py_engine import run_query

    n = 300_000
    _write(tmp_path / "b.bin", [("bk", T.INTEGER)], [np.arange(1000, dtype=np.int32)], 500)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("g", T.INTEGER)],
           [(np.arange(n) % 1000).astype(np.int32), np.arange(n, dtype=np.int32)], 1 << 16)
    api = _oracle_api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                 on=C("bk") == C("pk"), how="inner")
            .group_by(C("g")).agg(F.count())).task
    want = run_query(task)
    assert len(want) == n
    runs, stats = _run(tmp_path, task, hbm_tier=True)
    for rows in runs:
        assert_rows_match(rows, want, max_ulps=0)
    assert stats["tier"] == "hbm" and stats["partial_rows"] == n and stats["aggregate"] == "gathered", stats
    with pytest.raises(HipSparkError, match="on-chip"):
        _run(tmp_path, task, hbm_tier=False, runs=1)


def test_duplicate_keys_a_where_per_side_and_columns_of_both_sides(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from oracle.py_engine import run_query

    rng = np.random.default_rng(31)
    nb, npr = 120_000, 200_000
    bk = rng.integers(0, 60_000, nb).astype(np.int32)            # every key about twice on the build side
    bg = rng.integers(0, 50_000, nb).astype(np.int32)            # the GROUP BY column: ~50 000 values
    bi = rng.integers(-1000, 1000, nb).astype(np.int32)
    pk = rng.integers(0, 60_000, npr).astype(np.int32)           # ... and three times on the probe side
    pf = rng.normal(0, 100, npr).astype(np.float32)
    pw = rng.integers(0, 10, npr).astype(np.int32)
    _write(tmp_path / "b.bin", [("bk", T.INTEGER), ("bg", T.INTEGER), ("bi", T.INTEGER)], [bk, bg, bi], 50_000)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("pf", T.FLOAT), ("pw", T.INTEGER)], [pk, pf, pw], 1 << 16)
    api = _oracle_api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).filter(C("bi") > -900)
            .join(api.DataFrame().table(str(tmp_path / "p.bin")).filter(C("pw") != 3), on=C("bk") == C("pk"), how="inner")
            .group_by(C("bg")).agg(F.sum(C("pf")).alias("s"), F.max(C("bi")).alias("m"))).task
    want = run_query(task)
    assert len(want) > 40_000
    runs, stats = _run(tmp_path, task, hbm_tier=True)
    for rows in runs:
        assert_rows_match(rows, want, max_ulps=0)
    assert stats["tier"] == "hbm", stats


def test_a_dictionary_coded_string_key_on_the_hbm_tier(tmp_path):
    """A variable-length STRING GROUP BY key travels as one code byte and is decoded in the result file.  250 names over 32
    JoinJobs are 8 000 partial rows of five aggregates - more than the on-chip final merge takes - so the stage moves to the HBM
    tier on the number of partial ROWS, not of groups.  INTEGER aggregates only: their sums do not depend on how many JoinJobs fold them,
    so the oracle's ten partitions give the same rows."""
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.io import StrCol
    from oracle.py_engine import run_query

    rng = np.random.default_rng(41)
    nb, npr = 30_000, 90_000
    names = [("name-%d" % v) + "x" * (v % 9) for v in rng.integers(0, 250, nb)]
    _write(tmp_path / "b.bin", [("bk", T.INTEGER), ("bn", T.STRING)], [np.arange(nb, dtype=np.int32), StrCol.from_strings(names)], 8_000)
    _write(tmp_path / "p.bin", [("pk", T.INTEGER), ("pi", T.INTEGER)],
           [rng.integers(0, nb, npr).astype(np.int32), rng.integers(-1000, 1000, npr).astype(np.int32)], 1 << 15)
    api = _oracle_api()
    C, F = api.Col, api.F
    task = (api.DataFrame().table(str(tmp_path / "b.bin")).join(api.DataFrame().table(str(tmp_path / "p.bin")),
                                                                 on=C("bk") == C("pk"), how="inner")
            .group_by(C("bn")).agg(F.count(), F.sum(C("pi")).alias("s"), F.max(C("pi")).alias("m"), F.min(C("pi")).alias("lo"),
                                   F.sum(C("pi") * 2).alias("s2"))).task
    want = run_query(task)
    assert len(want) == 250
    runs, stats = _run(tmp_path, task, hbm_tier=True, n_parts=32)
    for rows in runs:
        assert_rows_match(rows, want, max_ulps=0)
    assert stats["tier"] == "hbm" and stats["dictionary"] == 250 and stats["partial_rows"] > 4096 and stats["result_rows"] == 250, stats
