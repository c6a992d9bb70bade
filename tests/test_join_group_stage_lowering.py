"""Lowering of a join feeding a GROUP BY into the plan blob of hs_join_group_stage (minispark_amd/stage.py
lower_join_group_stage_plan) and its ABI mirror, without a GPU: every supported shape lowers, every unsupported one is
refused before any device work."""

from __future__ import annotations

import ctypes as C

import pytest

from minispark_amd import hipspark as hs
from minispark_amd.stage import GROUP_KEY, StageUnsupported, lower_join_group_stage_plan
from tests.conftest import load_golden
from tests.queries import case_by_name
from tests.test_gpu_join_dict import _join_queries, _join_tables, _oracle_api
from tests.test_gpu_join_group_stage import _mixed_query, _mixed_tables


def test_the_plan_mirror_matches_the_library():
    lib = hs.load_library()
    assert lib.hs_sizeof(15) == C.sizeof(hs.hs_join_group_stage_plan)
    assert lib.hs_sizeof(13) == 0
    for name in ("prepare", "run", "stats", "destroy"):
        assert hasattr(lib, f"hs_join_group_stage_{name}")
    assert hasattr(lib, "hs_join_group_result_write_blockfile")


@pytest.mark.parametrize("name", ["join_group", "e2e_join_group_count", "e2e_join_group_sum"])
def test_golden_join_aggregates_lower(name):
    golden = load_golden(name)
    blob, build, probe, schema = lower_join_group_stage_plan(case_by_name(name).build(_oracle_api(), golden["paths"]).task)
    assert blob.version == hs.HS_JOIN_GROUP_STAGE_PLAN_VERSION and blob.n_parts == 10
    assert 1 <= blob.n_cols <= hs.HS_FUSED_COLS and 0 <= blob.key_slot < blob.n_cols
    assert blob.col_side[blob.key_slot] == 0  # every one of them groups by a build-side column
    assert build.exists() and probe.exists() and build != probe
    assert [blob.out_names[o].value.decode() for o in range(len(schema))] == [n.split(".")[-1] for n, _ in schema]


def test_having_after_the_join_is_refused():
    golden = load_golden("e2e_join_group_having")
    with pytest.raises(StageUnsupported, match="HAVING"):
        lower_join_group_stage_plan(case_by_name("e2e_join_group_having").build(_oracle_api(), golden["paths"]).task)


@pytest.mark.parametrize("name", ["config4", "filtered_with_build_side_argument", "probe_side_int_key",
                                  "filtered_on_the_probe_side", "count_only"])
def test_dictionary_join_queries_lower(tmp_path, name):
    orders, lineitem = _join_tables(tmp_path, 300, 2000, seed=21, dup=True)
    blob, *_ = lower_join_group_stage_plan(_join_queries(_oracle_api(), orders, lineitem)[name].task)
    sides = {blob.col_side[i] for i in range(blob.n_cols)}
    if name == "filtered_with_build_side_argument":
        assert sides == {0, 1}  # two build-side columns (key + o_totalprice) next to probe-side ones
        assert sum(blob.col_side[i] == 0 for i in range(blob.n_cols)) == 2
    if name.startswith("filtered"):
        assert blob.n_pcols >= 1 and blob.probe_filter.n_ins > 0  # one-side conjuncts go to that side's scan
    if name == "probe_side_int_key":
        assert blob.col_side[blob.key_slot] == 1


def test_shapes_of_the_generated_queries(tmp_path):
    b, p = _mixed_tables(tmp_path, nb=50, np_=200, block_rows=64)
    api = _oracle_api()
    cross, *_ = lower_join_group_stage_plan(_mixed_query(api, b, p, "cross_side_where").task)
    assert cross.n_pcols >= 1 and cross.n_bcols == 0  # pi < 250 is pushed; pf > bi * 10 stays in the aggregate
    assert cross.prog.n_ins > 0 and {cross.col_side[i] for i in range(cross.n_cols)} == {0, 1}
    strk, *_ = lower_join_group_stage_plan(_mixed_query(api, b, p, "string_keys").task)
    assert (strk.build_key_col, strk.probe_key_col) == (3, 5)
    ts, *_ = lower_join_group_stage_plan(_mixed_query(api, b, p, "probe_timestamp_key").task)
    assert (ts.col_side[ts.key_slot], ts.col_ids[ts.key_slot]) == (1, 2)
    bi, *_ = lower_join_group_stage_plan(_mixed_query(api, b, p, "build_int_key").task)
    assert (bi.col_side[bi.key_slot], bi.col_ids[bi.key_slot]) == (0, 2)
    ps, *_ = lower_join_group_stage_plan(_mixed_query(api, b, p, "probe_string_key").task)
    assert (ps.col_side[ps.key_slot], ps.col_ids[ps.key_slot]) == (1, 3) and ps.n_bcols == 1
    assert GROUP_KEY.startswith("__")


def test_refusals(tmp_path):
    from minispark_amd.constants import ColumnType as T
    from tests.test_gpu_join_select_stage import _write

    import numpy as np

    b, p = _mixed_tables(tmp_path, nb=50, np_=200, block_rows=64)
    api = _oracle_api()
    Col, F = api.Col, api.F

    def joined(on=None):
        return api.DataFrame().table(b).join(api.DataFrame().table(p), on=on if on is not None else Col("bk") == Col("pk"),
                                             how="inner")

    with pytest.raises(StageUnsupported, match="computed column"):
        lower_join_group_stage_plan(joined().select((Col("pf") * 2).alias("x"), Col("bs")).group_by(Col("bs"))
                                    .agg(F.sum(Col("x")).alias("s")).task)
    with pytest.raises(StageUnsupported, match="both INTEGER or both STRING"):
        lower_join_group_stage_plan(joined(Col("bk") == Col("pt")).group_by(Col("bs")).agg(F.count()).task)
    with pytest.raises(StageUnsupported, match="slots"):
        lower_join_group_stage_plan(joined().filter((Col("bs") != Col("pt")) & (Col("bt") != Col("ps"))).group_by(Col("bs")).agg(
            F.sum(Col("pf")).alias("a"), F.min(Col("bi")).alias("b"), F.max(Col("pi")).alias("c"), F.sum(Col("bk")).alias("d"),
            F.sum(Col("pk")).alias("e")).task)
    _write(tmp_path / "fb.bin", [("fk", T.FLOAT), ("g", T.INTEGER)], [np.ones(4, np.float32), np.arange(4, dtype=np.int32)], 4)
    _write(tmp_path / "fp.bin", [("fk2", T.FLOAT), ("v", T.INTEGER)], [np.ones(4, np.float32), np.arange(4, dtype=np.int32)], 4)
    with pytest.raises(StageUnsupported, match="FLOAT"):
        lower_join_group_stage_plan(api.DataFrame().table(str(tmp_path / "fb.bin")).join(
            api.DataFrame().table(str(tmp_path / "fp.bin")), on=Col("fk") == Col("fk2"), how="inner")
            .group_by(Col("g")).agg(F.sum(Col("v")).alias("s")).task)


def _pair_program():
    """The benchmark's aggregate (GROUP BY a coded build-side STRING, SUM(pf * bi), COUNT()) as hs_agg_shared's columns: the
    key gathered (one code byte per pair), pf and bi pair-indexed."""
    golden = load_golden("join_group")
    api = _oracle_api()
    Col, F = api.Col, api.F
    orders, lineitem = golden["paths"]["orders"], golden["paths"]["lineitem"]
    q = (api.DataFrame().table(orders).join(api.DataFrame().table(lineitem), on=Col("o_orderkey") == Col("l_orderkey"), how="inner")
         .group_by(Col("o_orderpriority")).agg(F.sum(Col("l_quantity") * Col("o_orderkey")).alias("w"), F.count()))
    blob, *_ = lower_join_group_stage_plan(q.task)
    cols = (hs.hs_col * blob.n_cols)()
    for i in range(blob.n_cols):
        if i == blob.key_slot:
            cols[i].kind, cols[i].fixed_len = hs.STR, 1
        else:
            cols[i].kind, cols[i].fixed_len = hs.PAIR | (hs.F32 if blob.col_side[i] else hs.I32), -1
    return blob, cols


def test_a_pair_indexed_program_translates_and_compiles_for_gfx950():
    lib = hs.load_library()
    blob, cols = _pair_program()
    src = C.create_string_buffer(1 << 16)
    nb = C.c_int64(0)
    rc = lib.hs_jit_compile_check_shared(cols, blob.n_cols, blob.key_slot, -1, C.byref(blob.prog), C.byref(blob.spec), b"gfx950",
                                         C.byref(nb), src, len(src))
    assert rc == 0, lib.hs_last_error()
    text = src.value.decode()
    assert nb.value > 0 and "TWO_STAGE = true" in text
    for i in range(blob.n_cols):
        if i != blob.key_slot:  # indices two steps ahead (load_keys), the values through them one step ahead (load)
            assert f"A.cols.c[{i}].offs + base" in text and f"d[x.ix{i}[3]]" in text and f"x.ix{i}[0] = k.ix{i}[0]" in text
    # the key is never pair-indexed
    cols[blob.key_slot].kind = hs.PAIR | hs.I32
    assert lib.hs_jit_compile_check_shared(cols, blob.n_cols, blob.key_slot, -1, C.byref(blob.prog), C.byref(blob.spec), b"gfx950",
                                           None, None, 0) != 0


def test_pair_indexed_columns_are_refused_without_the_jit():
    lib = hs.load_library()
    blob, cols = _pair_program()
    dummy = (C.c_uint64 * 64)()
    for i in range(blob.n_cols):
        cols[i].data = C.cast(dummy, C.c_void_p)
        if cols[i].kind & hs.PAIR:
            cols[i].offs = C.cast(dummy, C.c_void_p)
    units = (C.c_int64 * 3)(0, 50_000, 100_000)
    geom = hs.hs_agg_geom()
    assert lib.hs_agg_shared_geom(units, 2, blob.spec.n_acc, 16, C.byref(geom)) == 0 and geom.n_chunks > 0
    p = C.cast(dummy, C.c_void_p)
    was = lib.hs_jit_get_enabled()
    lib.hs_jit_set_enabled(0)
    try:
        rc = lib.hs_agg_shared(None, cols, blob.n_cols, blob.key_slot, C.byref(blob.prog), C.byref(blob.spec), p, 2, C.byref(geom),
                               p, p, p, p, p, None, None)
    finally:
        lib.hs_jit_set_enabled(was)
    assert rc == 2 and b"run-time compiler" in lib.hs_last_error()  # HS_E_LIMIT, before any launch
    pgeom = hs.hs_agg_geom()
    assert lib.hs_agg_partial_geom(units, 2, blob.spec.n_acc, 4, C.byref(pgeom)) == 0
    rc = lib.hs_agg_partial(None, cols, blob.n_cols, blob.key_slot, C.byref(blob.prog), C.byref(blob.spec), p, p, 2, C.byref(pgeom),
                            p, p, p, p, p, None, None)
    assert rc == 1 and b"HS_PAIR" in lib.hs_last_error()  # HS_E_ARG: the interpreter kernels never read them
