"""Narrow column kinds (HS_I64_FOR16 / HS_F32_LUT8) without a GPU: which slots of a fused scan read the
narrow side form, what the launch cache key is made of, and that the generated Q1 kernel with narrow slots compiles
for gfx950 under a cache key of its own."""

from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import pytest

from minispark_amd import hipspark as hs
from minispark_amd.device import DBatch, DCol, Device
from tests.conftest import load_golden


class _Tensor:
    """Stands in for a device tensor where only its address matters."""

    def __init__(self, ptr: int) -> None:
        self.ptr = ptr

    def data_ptr(self) -> int:
        return self.ptr


def _col(kind: int, n: int, ptr: int, narrow: DCol | None = None, **kw) -> DCol:
    return DCol(kind, _Tensor(ptr), n, narrow=narrow, **kw)


def _narrow(kind: int, n: int, ptr: int, entries: int = -1) -> DCol:
    return DCol(kind, _Tensor(ptr), n, offs=_Tensor(ptr + 8), fixed_len=entries)


def _q1_batch(n: int = 1000) -> DBatch:
    """The Q1 column set: three FLOAT columns and the date with narrow forms, the price without, the flag as the key."""
    cols = [
        _col(hs.F32, n, 0x1000, _narrow(hs.F32_LUT8, n, 0x9000, 50)),   # l_quantity
        _col(hs.F32, n, 0x2000),                                        # l_extendedprice: too many values
        _col(hs.F32, n, 0x3000, _narrow(hs.F32_LUT8, n, 0xa000, 11)),   # l_discount
        _col(hs.F32, n, 0x4000, _narrow(hs.F32_LUT8, n, 0xb000, 9)),    # l_tax
        _col(hs.STR, n, 0x5000, fixed_len=1, lens=_Tensor(0x5800)),     # l_returnflag
        _col(hs.I64, n, 0x6000, _narrow(hs.I64_FOR16, n, 0xc000)),      # l_shipdate
    ]
    schema = [(name, None) for name in ("q", "p", "d", "t", "f", "s")]
    return DBatch(schema, cols, n, [0, n])


def _device(enabled: bool = True) -> Device:
    dev = Device.__new__(Device)  # no GPU: only the pure-Python helpers are used
    dev.narrow_enabled = enabled
    return dev


def test_only_argument_slots_with_a_side_form_go_narrow():
    batch = _q1_batch()
    order = [0, 1, 2, 3, 4, 5]
    dev = _device()
    assert dev._narrow_slots(batch, order, (), 4) == [0, 2, 3, 5]
    assert Device._moved_bytes_per_row(batch, order, [0, 2, 3, 5]) == 10
    assert Device._moved_bytes_per_row(batch, order, []) == 25
    # the key slot never goes narrow, even when its column has a side form (GROUP BY l_quantity)
    assert dev._narrow_slots(batch, order, (), 0) == [2, 3, 5]
    # keyless tier: no key slot at all
    assert dev._narrow_slots(batch, order, (), None) == [0, 2, 3, 5]
    # switched off: the stored columns
    assert _device(False)._narrow_slots(batch, order, (), 4) == []
    # a slot beyond the preloaded ones stays plain
    many = list(range(6)) * 2
    assert all(s < hs.HS_FUSED_COLS for s in dev._narrow_slots(batch, many, (), 4))
    # a side form over other rows than the column's (a stale attachment) is not used
    batch.cols[0].narrow.n = 999
    assert dev._narrow_slots(batch, order, (), 4) == [2, 3, 5]
    # a variable-length string among the slots: no bytes-per-row figure
    batch.cols[4].fixed_len = -1
    assert Device._moved_bytes_per_row(batch, order, []) is None


def test_the_column_table_names_the_narrow_form_with_its_parameters():
    batch = _q1_batch()
    dev = _device()
    arr = dev._cols_array(batch, [0, 1, 2, 3, 4, 5], (), [0, 2, 3, 5])
    assert [arr[s].kind for s in range(6)] == [hs.F32_LUT8, hs.F32, hs.F32_LUT8, hs.F32_LUT8, hs.STR, hs.I64_FOR16]
    assert arr[0].data == 0x9000 and arr[0].offs == 0x9008 and arr[0].fixed_len == 50
    assert arr[5].data == 0xc000 and arr[5].offs == 0xc008
    assert arr[1].data == 0x2000 and arr[4].data == 0x5000  # the others as stored
    plain = dev._cols_array(batch, [0, 1, 2, 3, 4, 5], ())
    assert [plain[s].kind for s in range(6)] == [hs.F32, hs.F32, hs.F32, hs.F32, hs.STR, hs.I64]
    assert C.sizeof(hs.hs_col) == 32  # the decode parameters travel in existing fields


def test_a_derived_column_does_not_carry_the_side_form():
    col = _q1_batch().cols[0]
    assert DCol(col.kind, col.data, 10).narrow is None


def test_the_engine_switch_is_part_of_its_settings_and_keys(monkeypatch):
    from minispark_amd.execution import HipExecutionEngine

    eng = HipExecutionEngine.__new__(HipExecutionEngine)
    eng.dev = SimpleNamespace(narrow_enabled=True, zero_copy_results=True, timing_epoch=0)
    for name in ("replay_enabled", "short_tail_enabled", "shared_tier_enabled", "dict_enabled", "fused_join_enabled",
                 "fused_probe_enabled", "sharded_build_enabled"):
        setattr(eng, name, True)
    on = eng._switches()
    eng.narrow_enabled = False
    assert eng.dev.narrow_enabled is False and eng._switches() != on
    # the recording key: the switch and the side forms' buffers
    eng._tables, eng._caps, eng._global_partial, eng._global_merge = {}, {"group": 4, "merge": 16}, set(), set()
    plan = SimpleNamespace(_hs_scan_keys=["t"], stages=[])
    table = SimpleNamespace(columns={0: _q1_batch().cols[0]})
    eng._tables["t"] = table
    k_off = eng._recording_key(plan)
    eng.narrow_enabled = True
    k_on = eng._recording_key(plan)
    table.columns[0].narrow = None
    assert len({k_off, k_on, eng._recording_key(plan)}) == 3


def _q1_program():
    from minispark_amd.constants import ColumnType as T
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.plan import PhysicalPlan
    from minispark_amd.sql import Col, Functions, Lit
    from tests.queries import api_namespace, q1

    g = load_golden("q1_multiblock")
    api = api_namespace(lambda: DataFrame(engine=object()), Col, Functions, Lit)
    st = PhysicalPlan.generate_physical_plan(q1(api, g["paths"]["lineitem"]).task).stages[0]
    schema = st.producer.inferred_schema
    kind_of = {T.INTEGER: hs.I32, T.FLOAT: hs.F32, T.STRING: hs.STR, T.TIMESTAMP: hs.I64}
    kinds = [kind_of[t] for _, t in schema]
    low = lower_aggregate(schema, kinds, [st.consumers[0].condition], st.consumers[1].group_by_column,
                          st.consumers[1].agg_columns)
    return schema, kinds, low


def _q1_cols(schema, kinds, low, narrow: dict[str, tuple[int, int]], dummy):
    cols = (hs.hs_col * len(low.program.columns))()
    for slot, ci in enumerate(low.program.columns):
        name = schema[ci][0].split(".")[-1]
        cols[slot].kind = kinds[ci]
        cols[slot].fixed_len = 1 if kinds[ci] == hs.STR else -1
        if name in narrow and slot != low.key_slot:
            cols[slot].kind, cols[slot].fixed_len = narrow[name]
            cols[slot].data = C.cast(dummy, C.c_void_p)
            cols[slot].offs = C.cast(dummy, C.c_void_p)
    return cols


Q1_NARROW = {"l_quantity": (hs.F32_LUT8, 50), "l_discount": (hs.F32_LUT8, 11), "l_tax": (hs.F32_LUT8, 9),
             "l_shipdate": (hs.I64_FOR16, -1)}


def _key(lib, cols, low) -> str:
    out = C.create_string_buffer(8192)
    prog, spec = low.program.to_struct(), low.spec()
    assert lib.hs_jit_program_key(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), out, len(out)) == 0
    return out.value.decode()


def test_q1_with_narrow_slots_compiles_for_gfx950_under_its_own_cache_key():
    lib = hs.load_library()
    schema, kinds, low = _q1_program()
    dummy = (C.c_uint64 * 64)()
    cols = _q1_cols(schema, kinds, low, Q1_NARROW, dummy)
    assert sorted(cols[s].kind for s in range(len(low.program.columns))) == sorted(
        [hs.F32, hs.F32_LUT8, hs.F32_LUT8, hs.F32_LUT8, hs.STR, hs.I64_FOR16])
    prog, spec = low.program.to_struct(), low.spec()
    src = C.create_string_buffer(1 << 16)
    nbytes = C.c_int64(0)
    rc = lib.hs_jit_compile_check(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                  C.byref(nbytes), src, len(src))
    assert rc == 0, (lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
    assert nbytes.value > 4096
    text = src.value.decode()
    assert "HAS_TABLES = true" in text and "load_tables" in text and "store_tables" in text
    # the value tables are sized to the power of two that covers the entry count: 64 + 16 + 16 f64 entries, under 1 KiB
    assert text.count("__shared__ double hs_lut_c") == 3
    assert "[64];" in text and text.count("[16];") == 2 and "__shared__ unsigned long long hs_for_c" in text
    # cut and decoded in run(), never in load(): load() keeps the words as loaded
    load_body = text.split("void load(")[1].split("template <class Ctx>")[0]
    assert "hs_lut_c" not in load_body and "for" + "5_b" not in load_body and ">>" not in load_body
    assert load_body.count("__builtin_nontemporal_load") >= 5
    # same aggregate code as the plain kernel
    assert "hs_agg_main_body<JitProg>" in text and text.count("= hs_acc_fold(") == 6

    plain = _q1_cols(schema, kinds, low, {}, dummy)
    k_plain, k_narrow = _key(lib, plain, low), _key(lib, cols, low)
    assert k_plain != k_narrow
    # the table SIZE CLASS is compiled in (not the entry count): 9 and 11 entries share a program, 11 and 50 do not
    same = dict(Q1_NARROW, l_tax=(hs.F32_LUT8, 11))
    other = dict(Q1_NARROW, l_discount=(hs.F32_LUT8, 50))
    assert _key(lib, _q1_cols(schema, kinds, low, same, dummy), low) == k_narrow
    assert _key(lib, _q1_cols(schema, kinds, low, other, dummy), low) != k_narrow
    # the plain kernel's source is what it was: no tables, no extra LDS
    rc = lib.hs_jit_compile_check(plain, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                  C.byref(nbytes), src, len(src))
    assert rc == 0
    assert "HAS_TABLES = false" in src.value.decode() and "__shared__" not in src.value.decode()


def test_a_narrow_key_or_a_shared_tier_program_is_refused_by_the_translator():
    lib = hs.load_library()
    schema, kinds, low = _q1_program()
    dummy = (C.c_uint64 * 64)()
    cols = _q1_cols(schema, kinds, low, Q1_NARROW, dummy)
    prog, spec = low.program.to_struct(), low.spec()
    assert lib.hs_jit_compile_check_shared(cols, len(low.program.columns), low.key_slot, -1, C.byref(prog), C.byref(spec),
                                           b"gfx950", None, None, 0) != 0
    assert b"narrow" in lib.hs_last_error()
    # a value table without entries / with more than a code byte names
    for entries in (0, 257):
        bad = _q1_cols(schema, kinds, low, dict(Q1_NARROW, l_tax=(hs.F32_LUT8, entries)), dummy)
        assert lib.hs_jit_compile_check(bad, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                        None, None, 0) != 0


@pytest.mark.parametrize("entry", ["hs_eval", "hs_order_by", "hs_distinct", "hs_key_pack"])
def test_other_entry_points_refuse_narrow_columns_before_any_launch(entry):
    """HS_E_ARG with a message, decided on the host before anything touches a device."""
    lib = hs.load_library()
    dummy = (C.c_uint64 * 64)()
    col = (hs.hs_col * 1)()
    col[0].kind, col[0].fixed_len = hs.F32_LUT8, 4
    col[0].data = col[0].offs = C.cast(dummy, C.c_void_p)
    p = C.cast(dummy, C.c_void_p)
    if entry == "hs_eval":
        prog = hs.hs_program()
        kinds = (C.c_int32 * 1)(hs.F64)
        outs = (C.c_void_p * 1)(p)
        rc = lib.hs_eval(None, col, 1, C.byref(prog), None, 8, None, outs, kinds, 1, p)
    elif entry == "hs_order_by":
        desc = (C.c_int32 * 1)(0)
        count = C.c_int64(0)
        rc = lib.hs_order_by(None, col, desc, 1, 8, None, -1, p, C.byref(count), p, p)
    elif entry == "hs_distinct":
        count = C.c_int64(0)
        rc = lib.hs_distinct(None, col, 1, 8, None, p, C.byref(count), p, p)
    else:
        rc = lib.hs_key_pack(None, col, 1, 8, p, 4)
    assert rc == 1  # HS_E_ARG
    assert b"narrow" in lib.hs_last_error()
