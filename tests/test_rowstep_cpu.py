"""The generated private-tier scan without a GPU (DESIGN.md 4.1 "a quad at a time", 4.5a): which programs get the batched
slot resolution and the compare on the frame-of-reference delta, which keep the row-at-a-time form, and that all of them
compile for gfx950."""

from __future__ import annotations

import ctypes as C
import re

from minispark_amd import hipspark as hs
from tests.test_narrow_cpu import Q1_NARROW, _q1_cols, _q1_program

DECODE = re.compile(r"for\d+_b \+ .*\* for\d+_s")  # base + delta * scale


def _compile(cols, program, spec, key_slot: int, scalar: bool = False) -> str:
    lib = hs.load_library()
    prog = program.to_struct()
    src = C.create_string_buffer(1 << 16)
    nbytes = C.c_int64(0)
    if scalar:
        rc = lib.hs_jit_compile_check_scalar(cols, len(program.columns), C.byref(prog), C.byref(spec), b"gfx950",
                                             C.byref(nbytes), src, len(src))
    else:
        rc = lib.hs_jit_compile_check(cols, len(program.columns), key_slot, C.byref(prog), C.byref(spec), b"gfx950",
                                      C.byref(nbytes), src, len(src))
    assert rc == 0, (lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
    assert nbytes.value > 4096
    return src.value.decode()


def _q1(narrow: bool):
    schema, kinds, low = _q1_program()
    dummy = (C.c_uint64 * 64)()
    return low, _q1_cols(schema, kinds, low, Q1_NARROW if narrow else {}, dummy), dummy


def test_narrow_q1_resolves_the_quad_up_front_and_never_decodes_the_date():
    low, cols, _keep = _q1(narrow=True)
    text = _compile(cols, low.program, low.spec(), low.key_slot)
    run = text.split("void load(")[1].split("template <class Ctx>")
    assert len(run) == 2, "one `template <class Ctx>` after load(): the interior variant rides in the type of Ctx"
    run = run[1]
    assert text.count("= hs_acc_fold(") == 6, "the fold is emitted once"
    assert not DECODE.search(text) and "hs_for16_threshold(" in text
    assert re.search(r"& 0xffffu\) < for\d+_t0", run), "l_shipdate <= literal, on the delta"
    # {base, scale, threshold}: one more LDS word than before
    assert re.search(r"__shared__ unsigned long long hs_for_c\d+\[3\];", text)
    # four map reads, one wave-level branch, the row-order find in its cold arm only
    assert run.count("ctx.dmap[") == 1 and "__any(miss)" in run and run.count("find_byte_small(") == 1
    assert "ctx.find_byte(" not in run
    assert run.index("__any(miss)") < run.index("hs_lut_c") < run.index("= hs_acc_fold(")
    # each table is read once per row, in one batch per table
    assert len(re.findall(r"= hs_lut_c\d+\[", run)) == 3
    assert "Ctx::ALL_ALIVE || ctx.alive[j]" in run and "INTERIOR_STEPS = true" in text
    assert "__umul24((unsigned)slot, 1536u)" in run  # 6 accumulators x 256 lanes: the cell's address in 32 bits


def test_plain_q1_gets_the_same_shape_and_no_static_lds():
    low, cols, _keep = _q1(narrow=False)
    text = _compile(cols, low.program, low.spec(), low.key_slot)
    assert "__shared__" not in text and "HAS_TABLES = false" in text
    assert "__any(miss)" in text and text.count("= hs_acc_fold(") == 6
    assert text.count("template <class Ctx>") == 1


def test_a_filter_after_the_key_keeps_the_row_at_a_time_form():
    low, cols, _keep = _q1(narrow=True)
    ins = list(low.program.ins)
    at = [w & 0xFF for w in ins].index(hs.OP_KEY)
    assert [w & 0xFF for w in ins[:at]][-1] == hs.OP_FILTER and ((ins[at] >> 8) & 0xFF) == 0
    low.program.ins = [ins[at]] + ins[:at] + ins[at + 1:]  # KEY, then the WHERE (the stack is empty at both places)
    text = _compile(cols, low.program, low.spec(), low.key_slot)
    assert "__any(miss)" not in text and "ctx.find_byte(" in text
    assert not DECODE.search(text), "the compare on the delta does not depend on the batched form"
    assert text.count("= hs_acc_fold(") == 6


def test_a_two_byte_key_keeps_the_row_at_a_time_form():
    low, cols, _keep = _q1(narrow=True)
    cols[low.key_slot].fixed_len = 2
    text = _compile(cols, low.program, low.spec(), low.key_slot)
    assert "__any(miss)" not in text and "ctx.template find<HASHED>(" in text
    assert "Ctx::ALL_ALIVE || ctx.alive[j]" in text  # interior steps are a matter of the tier, not of the key


def _lineitem():
    from minispark_amd.constants import ColumnType as T

    schema = [("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT), ("l_discount", T.FLOAT), ("l_returnflag", T.STRING),
              ("l_shipdate", T.TIMESTAMP)]
    return schema, [hs.F32, hs.F32, hs.F32, hs.STR, hs.I64]


def _cols_of(low, kinds, dummy):
    cols = (hs.hs_col * len(low.program.columns))()
    for slot, ci in enumerate(low.program.columns):
        cols[slot].kind = kinds[ci]
        cols[slot].fixed_len = 1 if kinds[ci] == hs.STR else -1
        if kinds[ci] == hs.I64:
            cols[slot].kind = hs.I64_FOR16
            cols[slot].data = cols[slot].offs = C.cast(dummy, C.c_void_p)
    return cols


def test_a_second_use_of_the_decoded_date_keeps_the_decode():
    from datetime import datetime

    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.sql import Col, Functions as F, Lit

    schema, kinds = _lineitem()
    cond = Col("l_shipdate") <= Lit(datetime(1998, 9, 2))
    dummy = (C.c_uint64 * 64)()
    for aggs, decoded in (([F.sum(Col("l_quantity"))], False), ([F.sum(F.year(Col("l_shipdate")))], True)):
        low = lower_aggregate(schema, kinds, [cond], Col("l_returnflag"), aggs)
        text = _compile(_cols_of(low, kinds, dummy), low.program, low.spec(), low.key_slot)
        assert bool(DECODE.search(text)) == decoded
        assert re.search(r"< for\d+_t0", text), "the WHERE's own load is compared on the delta either way"
    # == and != decode as before
    low = lower_aggregate(schema, kinds, [Col("l_shipdate") != Lit(datetime(1998, 9, 2))], Col("l_returnflag"),
                          [F.sum(Col("l_quantity"))])
    text = _compile(_cols_of(low, kinds, dummy), low.program, low.spec(), low.key_slot)
    assert DECODE.search(text) and "hs_for16_threshold(" not in text


def test_the_keyless_kernel_compares_on_the_delta_in_both_operand_orders():
    from datetime import datetime

    from minispark_amd.lowering import lower_aggregate
    from minispark_amd.sql import Col, Functions as F, Lit

    schema, kinds = _lineitem()
    conds = [(Col("l_shipdate") >= Lit(datetime(1994, 1, 1))) & (Lit(datetime(1995, 1, 1)) > Col("l_shipdate"))]
    low = lower_aggregate(schema, kinds, conds, None, [F.sum(Col("l_extendedprice") * Col("l_discount"))])
    dummy = (C.c_uint64 * 64)()
    text = _compile(_cols_of(low, kinds, dummy), low.program, low.spec(), -1, scalar=True)
    assert "hs_agg_scalar_body<JitProg>" in text and not DECODE.search(text)
    # value >= literal: strict threshold, d >= T;  literal > value is value < literal: strict threshold, d < T
    assert re.search(r">= for\d+_t0", text) and re.search(r"< for\d+_t1", text)
    assert text.count("hs_for16_threshold(") == 2 and text.count(", true);") == 2
    assert re.search(r"__shared__ unsigned long long hs_for_c\d+\[4\];", text)
    assert "ALL_ALIVE" not in text and "INTERIOR_STEPS = false" in text  # the keyless skeleton is what it was


def test_the_cache_key_version_follows_the_generated_text():
    lib = hs.load_library()
    low, cols, _keep = _q1(narrow=True)
    out = C.create_string_buffer(8192)
    prog, spec = low.program.to_struct(), low.spec()
    assert lib.hs_jit_program_key(cols, len(low.program.columns), low.key_slot, C.byref(prog), C.byref(spec), out, len(out)) == 0
    assert "|v14|" in "|" + out.value.decode()
