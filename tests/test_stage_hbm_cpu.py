"""Host-only parts of the HBM tier behind the native stages: the switches refuse a null stage, the row-forming pass sizes its
workspace and classifies aggregate arguments from the program alone (no GPU)."""

from __future__ import annotations

import ctypes as C

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType as T
from minispark_amd.lowering import lower_aggregate
from minispark_amd.sql import Col, Functions as F, Lit


def test_the_switches_and_reports_refuse_a_null_stage():
    lib = hs.load_library()
    out = (C.c_int64 * 4)()
    assert lib.hs_stage_set_hbm_tier(None, 1) == 1 and b"hs_stage_set_hbm_tier" in lib.hs_last_error()
    assert lib.hs_join_group_stage_set_hbm_tier(None, 1) == 1
    assert lib.hs_stage_tier_stats(None, out) == 1 and lib.hs_join_group_stage_tier_stats(None, out) == 1


def test_workspace_of_the_row_forming_pass_grows_with_its_arguments():
    lib = hs.load_library()
    sizes = [lib.hs_agg_rows_ws_bytes(n, u) for n, u in [(0, 0), (1, 1), (10**6, 1), (10**6, 300), (6 * 10**7, 29), (6 * 10**7, 5000)]]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[2] < sizes[3] and sizes[4] < sizes[5]
    assert lib.hs_agg_rows_ws_bytes(-5, -1) == sizes[0]  # negative arguments count as zero
    assert sizes[4] < 1 << 20  # one count and one start per 4096-row segment: far below a column


def _classify(filters, aggs, key="k"):
    lib = hs.load_library()
    schema = [("k", T.INTEGER), ("f", T.FLOAT), ("i", T.INTEGER), ("t", T.TIMESTAMP)]
    kinds = [hs.I32, hs.F32, hs.I32, hs.I64]
    low = lower_aggregate(schema, kinds, filters, Col(key), aggs)
    cols = (hs.hs_col * len(low.program.columns))(*[hs.hs_col(kinds[idx], -1, None, None, None) for idx in low.program.columns])
    prog, spec = low.program.to_struct(), low.spec()
    vk, vs, cc, nf = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_uint64 * 16)(), C.c_int32(-1)
    hs.check(lib.hs_agg_rows_classify(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), vk, vs, cc, C.byref(nf)))
    accs = [low.agg_to_acc[j] for j in range(len(aggs))]
    return [(int(vk[a]), low.program.columns[vs[a]] if vs[a] >= 0 else -1, int(cc[a])) for a in accs], nf.value


def test_arguments_travel_as_literal_stored_column_or_cell():
    got, n_filters = _classify([Col("i") > 3, Col("f") < 2.0],
                               [F.count(), F.sum(Col("f")).alias("a"), F.min(Col("i")).alias("b"),
                                F.sum(Col("f") * (Lit(1) - Col("f"))).alias("d"), F.sum(Col("i") * 2).alias("e")])
    assert n_filters == 2
    assert got[0] == (-1, -1, 1)             # COUNT's 1: nothing travels, the cell goes to the radix run
    assert got[1] == (hs.F32, 1, 0)          # bare stored columns in their stored width, by table column
    assert got[2] == (hs.I32, 2, 0)
    assert got[3] == (hs.F64, -1, 0)         # expressions as the interpreter's cells
    assert got[4] == (hs.I64, -1, 0)
    assert _classify([], [F.count()])[1] == 0


def test_a_program_without_the_stage_shape_is_refused():
    lib = hs.load_library()
    prog, spec = hs.hs_program(), hs.hs_agg_spec()
    cols = (hs.hs_col * 1)(hs.hs_col(hs.I32, -1, None, None, None))
    vk, vs, cc = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_uint64 * 16)()
    assert lib.hs_agg_rows_classify(cols, 1, 0, C.byref(prog), C.byref(spec), vk, vs, cc, None) == 1  # no KEY instruction
    assert b"KEY" in lib.hs_last_error()
    assert lib.hs_agg_rows(None, cols, 1, 0, C.byref(prog), C.byref(spec), None, 1, 10, None, None, None, None, None, None) == 1
