"""Which route a join whose probe side exceeds the HBM budget takes (host logic, no GPU): the join stage reads the
probe side range by range when it writes the result file or feeds the short-tail GROUP BY through WHERE conditions
only; every other join - and one a run has refused (execution.probe_side_streams) - has its probe side streamed,
concatenated and joined resident.  The shapes are those of tests/test_gpu_streamed_joins.py."""

from __future__ import annotations

import pytest

from minispark_amd.execution import HipExecutionEngine, _cls, _uid, probe_side_streams
from minispark_amd.plan import PhysicalPlan
from tests.test_gpu_join_dict import _join_queries, _join_tables, _oracle_api
from tests.test_gpu_streamed_joins import MATRIX, _case, _orders_lineitem_to_file

# range by range unless a run refuses it (True), or resident from the plan alone (False)
PLANNED = {
    "build_side_argument": True, "dup_build_keys": True, "sparse_int_keys_group": True, "sparse_int_keys_to_file": True,
    "string_keys_group": True, "string_keys_to_file": True, "projection_before_group_by": False,
    "many_string_group_keys": True, "float_group_key": True, "chain_group": False, "chain_to_file": False,
}


def _probe_joins(plan):
    """Join stages whose probe (right) side is a table scan."""
    return [st for st in plan.stages if _cls(st.producer) == "BroadcastHashJoinTask" and len(st.dependencies) == 2
            and _cls(st.dependencies[1].producer) == "LoadTableBlockTask"]


def _plan(frame):
    plan = PhysicalPlan.generate_physical_plan(frame.task)
    HipExecutionEngine._mark_short_tails(plan)  # what the engine does to every plan it caches
    return plan


def test_every_matrix_shape_has_a_planned_route():
    assert sorted(PLANNED) == sorted(MATRIX)


@pytest.mark.parametrize("name", MATRIX)
def test_route_of_the_streamed_matrix(tmp_path, name):
    build = _case(name, tmp_path)[0]
    (join,) = _probe_joins(_plan(build(_oracle_api())))
    assert probe_side_streams(join, set(), set()) is PLANNED[name]
    # a join a run refused never streams range by range again
    assert probe_side_streams(join, {_uid(join.producer)}, set()) is False
    to_file = _cls(join.writer) == "WriteToLocalFileTask"
    # the byte table turned out not to hold this join: only the result-file form still streams range by range
    assert probe_side_streams(join, set(), {_uid(join.producer)}) is (PLANNED[name] and to_file)
    assert probe_side_streams(join, {object()}, {object()}) is PLANNED[name]
    # ... nor once its GROUP BY lost the short tail (the byte table's probe runs inside it)
    first_real = next((t for t in join.consumers if _cls(t) != "FilterTask"), None)
    if first_real is not None:
        assert probe_side_streams(join, set(), {_uid(first_real)}) is (PLANNED[name] and to_file)


@pytest.mark.parametrize("name", ["config4", "filtered_on_the_probe_side", "count_only", "probe_side_int_key", "to_file"])
def test_byte_table_joins_and_joins_to_file_stream_range_by_range(tmp_path, name):
    orders, lineitem = _join_tables(tmp_path, 300, 900, seed=1)
    api = _oracle_api()
    frame = _orders_lineitem_to_file(api, orders, lineitem) if name == "to_file" else _join_queries(api, orders, lineitem)[name]
    (join,) = _probe_joins(_plan(frame))
    assert probe_side_streams(join, set(), set()) is True


def test_a_join_feeding_another_join_is_joined_resident(tmp_path):
    """customers JOIN (orders JOIN lineitem): the inner join writes a shuffle that the outer join reads as its probe
    side - neither a GROUP BY nor the result file."""
    build = _case("chain_group", tmp_path)[0]
    plan = _plan(build(_oracle_api()))
    joins = [st for st in plan.stages if _cls(st.producer) == "BroadcastHashJoinTask"]
    assert len(joins) == 2
    (inner,) = _probe_joins(plan)
    assert _cls(inner.writer) == "WriteToShufflePartitions" and any(inner is dep for j in joins for dep in j.dependencies)
    assert probe_side_streams(inner, set(), set()) is False
