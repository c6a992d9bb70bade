"""minispark_amd/stage.py lower_join_select_stage_plan: [scan, scan, join -> result file] -> hs_join_select_stage_plan, on the
host alone (no GPU): the golden join queries lower, the binding's mirror has the library's size, unsupported shapes are refused."""

from __future__ import annotations

import ctypes as C

import pytest

from tests.conftest import load_golden
from tests.queries import case_by_name

GOLDENS = ["e2e_join_select", "e2e_join_where_float", "e2e_join_where_ts", "fruits5_self_join"]


def _api():
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col, Functions, Lit
    from minispark_amd.workloads import api_namespace

    return api_namespace(lambda: DataFrame(engine=object()), Col, Functions, Lit)


def test_plan_blob_size_matches_the_library():
    from minispark_amd import hipspark as hs

    lib = hs.load_library()
    assert lib.hs_sizeof(14) == C.sizeof(hs.hs_join_select_stage_plan)
    assert lib.hs_sizeof(13) == 0  # unassigned (tests/test_abi.py reads it as the end of the older list)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_join_queries_lower_to_a_plan_blob(name):
    from minispark_amd import hipspark as hs
    from minispark_amd.stage import lower_join_select_stage_plan

    g = load_golden(name)
    blob, build, probe, schema = lower_join_select_stage_plan(case_by_name(name).build(_api(), g["paths"]).task)
    assert blob.version == hs.HS_JOIN_SELECT_STAGE_PLAN_VERSION and blob.n_parts == 10
    assert [n for n, _ in schema] == [n for n, _ in g["schema"]]
    assert blob.n_out == len(schema)
    assert [blob.out_names[o].value.decode() for o in range(blob.n_out)] == [n for n, _ in g["schema"]]
    assert str(build) in g["paths"].values() and str(probe) in g["paths"].values()


def test_where_conjuncts_are_pushed_to_their_side():
    from minispark_amd.stage import lower_join_select_stage_plan

    g = load_golden("e2e_join_where_float")
    blob, *_ = lower_join_select_stage_plan(case_by_name("e2e_join_where_float").build(_api(), g["paths"]).task)
    assert blob.build_filter.n_ins == 0 and blob.probe_filter.n_ins > 0  # o.price > 100: the probe side (orders)
    g = load_golden("e2e_join_where_ts")
    blob, *_ = lower_join_select_stage_plan(case_by_name("e2e_join_where_ts").build(_api(), g["paths"]).task)
    assert blob.build_filter.n_ins > 0 and blob.probe_filter.n_ins == 0  # o.order_date: orders is the build side here
    assert list(blob.bcol_ids)[: blob.n_bcols] == [5]
    # two one-side conjuncts of one WHERE go to their two sides
    api = _api()
    C_ = api.Col
    u = api.DataFrame().table(g["paths"]["users"]).alias("u")
    o = api.DataFrame().table(g["paths"]["orders"]).alias("o")
    q = (u.join(o, on=C_("u.user_id") == C_("o.user_id"), how="inner")
         .filter((C_("u.age") > 30) & (C_("o.quantity") > 1)).select(C_("u.first_name"), C_("o.product")))
    blob, *_ = lower_join_select_stage_plan(q.task)
    assert blob.build_filter.n_ins > 0 and blob.probe_filter.n_ins > 0


def test_unsupported_shapes_are_refused_on_the_host():
    from minispark_amd.stage import StageUnsupported, lower_join_select_stage_plan

    g = load_golden("e2e_join_select")
    api = _api()
    C_, F = api.Col, api.F

    def u():
        return api.DataFrame().table(g["paths"]["users"]).alias("u")

    def o():
        return api.DataFrame().table(g["paths"]["orders"]).alias("o")

    def joined():
        return u().join(o(), on=C_("u.user_id") == C_("o.user_id"), how="inner")

    with pytest.raises(StageUnsupported):  # a join feeding GROUP BY is hs_join_stage
        lower_join_select_stage_plan(joined().group_by(C_("u.country")).agg(F.count().alias("n")).task)
    with pytest.raises(StageUnsupported, match="INTEGER or both STRING"):
        lower_join_select_stage_plan(u().join(o(), on=C_("u.user_id") == C_("o.product"), how="inner").task)
    with pytest.raises(StageUnsupported, match="both sides"):
        lower_join_select_stage_plan(joined().filter(C_("u.age") > C_("o.quantity")).select(C_("u.first_name")).task)
    with pytest.raises(StageUnsupported, match="computed column"):
        lower_join_select_stage_plan(joined().select((C_("o.quantity") * 2).alias("q2")).task)
    with pytest.raises(StageUnsupported, match="INTEGER or both STRING"):
        lower_join_select_stage_plan(u().join(o(), on=C_("u.user_id") == C_("o.order_date"), how="inner").task)
