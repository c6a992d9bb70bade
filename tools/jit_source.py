"""The HIP source the run-time compiler (csrc/hs_jit.hip) generates, without a GPU (hiprtc cross-compiles for gfx950).

    jit_source.py [--narrow]     the Q1 scan (private-table tier), with --narrow over the narrow column kinds
    jit_source.py --join         BASELINE config 4: the shared-dictionary scan with the join's probe inside
    jit_source.py --corpus DIR   one DIR/<name>.hip per program of the corpus below and DIR/MANIFEST: `name sha256`, or
                                 `name DECLINED: <text>` for a program the translator declines

A single program goes to stdout:  ... > q1.hip ; hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S
--cuda-device-only -Iinclude -Iminispark_amd/csrc q1.hip

The corpus reaches every arm of the two generators; two commits generate the same code when their manifests are equal.
Its programs come from the lowering and from the helpers of the CPU tests (tests/jit_programs.py and the tests named below)."""
import ctypes as C
import hashlib
import os
import sys
from datetime import datetime
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minispark_amd import hipspark as hs  # noqa: E402
from minispark_amd.lowering import ProgramBuilder, lower_aggregate  # noqa: E402
from minispark_amd.sql import Col, Functions as F, Lit  # noqa: E402
from tests import jit_programs as jp  # noqa: E402

_KEEP = []  # buffers the column tables point into


def _dummy():
    _KEEP.append((C.c_uint64 * 64)())
    return _KEEP[-1]


def q1(narrow: bool = False):
    """-> (cols, low): the Q1 stage as the engine lowers it (tests/test_narrow_cpu.py)."""
    from tests.test_narrow_cpu import Q1_NARROW, _q1_cols, _q1_program

    schema, kinds, low = _q1_program()
    return _q1_cols(schema, kinds, low, Q1_NARROW if narrow else {}, _dummy()), low


def join8():
    """-> (cols, n_cols, low): the GROUP BY key a HS_JOIN8_CODE column, the unit the HS_JOIN8_UNIT column behind the last slot."""
    from minispark_amd.constants import ColumnType as T

    schema = [("o_orderpriority", T.STRING), ("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT)]
    kinds = [hs.STR, hs.F32, hs.F32]
    dicts = [(b"1-URGENT", b"2-HIGH", b"3-MEDIUM", b"4-NOT SPECIFIED", b"5-LOW"), None, None]
    low = lower_aggregate(schema, kinds, [], Col("o_orderpriority"),
                          [F.count().alias("n"), F.sum(Col("l_quantity")).alias("qty"), F.sum(Col("l_extendedprice")).alias("revenue"),
                           F.max(Col("l_extendedprice")).alias("max_price")], dicts)
    n = len(low.program.columns)
    cols = (hs.hs_col * (n + 1))()
    for slot, ci in enumerate(low.program.columns):
        cols[slot].kind, cols[slot].fixed_len = (hs.JOIN8_CODE, 1) if kinds[ci] == hs.STR else (kinds[ci], -1)
    cols[n].kind, cols[n].fixed_len = hs.JOIN8_UNIT, -1
    return cols, n + 1, low


def agg_case(name, entry, cols, low, n_cols=None, unit=-1):
    n = len(low.program.columns) if n_cols is None else n_cols
    return name, entry, cols, n, low.program.to_struct(), low.spec(), (-1 if entry == "scalar" else low.key_slot), unit, 0


def _raw(name, entry, kinds, words, n_acc=1, key=0, unit=-1, fixed=None):
    """A hand-built program over a column table of `kinds` (`fixed`: slot -> fixed_len)."""
    cols = jp.columns(kinds)
    for slot, fl in (fixed or {}).items():
        cols[slot].fixed_len = fl
    for slot, kind in enumerate(kinds):
        if kind in (hs.I64_FOR16, hs.F32_LUT8):
            cols[slot].data = cols[slot].offs = C.cast(_dummy(), C.c_void_p)
    if entry == "eval":
        return name, entry, cols, len(kinds), jp.program(words), (C.c_int32 * 1)(hs.F64), -1, -1, 1
    return name, entry, cols, len(kinds), jp.program(words), jp.spec(n_acc), (-1 if entry == "scalar" else key), unit, 0


def corpus():
    """(name, entry point, cols, n_cols, hs_program, hs_agg_spec | out kinds, key slot, unit slot, outputs) per program."""
    from tests.test_date_parts_cpu import DICTS, KINDS, SCHEMA, _hs_cols  # a b INTEGER, f FLOAT, s d STRING (d coded), ts t2 TIMESTAMP
    from tests.test_join_group_stage_lowering import _pair_program
    from tests.test_rowstep_cpu import _cols_of, _lineitem

    w, op = jp.word, hs
    # ---- private-table tier
    for narrow in (False, True):
        cols, low = q1(narrow)
        yield agg_case("private_q1_" + ("narrow" if narrow else "plain"), "private", cols, low)
    cols, low = q1(True)  # the three row-at-a-time variants of tests/test_rowstep_cpu.py
    ins = list(low.program.ins)
    at = [x & 0xFF for x in ins].index(hs.OP_KEY)
    low.program.ins = [ins[at]] + ins[:at] + ins[at + 1:]
    yield agg_case("private_q1_filter_after_key", "private", cols, low)
    for width in (2, 4):
        cols, low = q1(True)
        cols[low.key_slot].fixed_len = width
        yield agg_case(f"private_q1_key{width}", "private", cols, low)
    aggs = [F.sum(Col("f")), F.count(), F.max(Col("b"))]
    for key in ("a", "f", "s"):  # INTEGER and FLOAT keys; a STRING of any length: the hashed tier, the key read per row
        low = lower_aggregate(SCHEMA, KINDS, [Col("b") > 3], Col(key), aggs, DICTS)
        cols = _hs_cols(low.program, KINDS)
        if key == "s":
            cols[low.key_slot].fixed_len = -1
        yield agg_case(f"private_key_{key}", "private", cols, low)
    schema, kinds = _lineitem()
    day = Lit(datetime(1998, 9, 2))
    for name, cond, agg in (("decoded_twice", Col("l_shipdate") <= day, F.sum(F.year(Col("l_shipdate")))),
                            ("eq", Col("l_shipdate") == day, F.sum(Col("l_quantity"))),
                            ("ne", Col("l_shipdate") != day, F.sum(Col("l_quantity")))):
        low = lower_aggregate(schema, kinds, [cond], Col("l_returnflag"), [agg])
        yield agg_case("private_for16_" + name, "private", _cols_of(low, kinds, _dummy()), low)
    # ---- shared-dictionary tier
    from minispark_amd.constants import ColumnType as T

    sschema = [("o_orderpriority", T.STRING), ("l_shipmode", T.STRING), ("l_quantity", T.FLOAT), ("l_extendedprice", T.FLOAT)]
    skinds = [hs.STR, hs.STR, hs.F32, hs.F32]
    sdicts = [(b"1-URGENT", b"2-HIGH"), (b"AIR", b"MAIL", b"REG AIR"), None, None]
    low = lower_aggregate(sschema, skinds, [Col("l_shipmode").like("%AIR%")], Col("o_orderpriority"),
                          [F.count().alias("n"), F.sum(Col("l_quantity")).alias("q"), F.max(Col("l_extendedprice")).alias("m")], sdicts)
    n = len(low.program.columns)
    cols = (hs.hs_col * (n + 1))()
    for slot, ci in enumerate(low.program.columns):
        cols[slot].kind, cols[slot].fixed_len = skinds[ci], (1 if skinds[ci] == hs.STR else -1)
    cols[n].kind, cols[n].fixed_len = hs.U8, -1
    yield agg_case("shared_no_unit", "shared", cols, low, n + 1)
    yield agg_case("shared_u8_unit", "shared", cols, low, n + 1, unit=n)
    cols, n, low = join8()
    yield agg_case("shared_join8", "shared", cols, low, n, unit=n - 1)
    blob, cols = _pair_program()
    yield "shared_pair", "shared", cols, blob.n_cols, blob.prog, blob.spec, blob.key_slot, -1, 0
    # ---- keyless tier
    low = lower_aggregate(SCHEMA, KINDS, [Col("b") > 3], None, aggs, DICTS)
    yield agg_case("scalar_global", "scalar", _hs_cols(low.program, KINDS), low)
    conds = [(Col("l_shipdate") >= Lit(datetime(1994, 1, 1))) & (Lit(datetime(1995, 1, 1)) > Col("l_shipdate"))]
    low = lower_aggregate(schema, kinds, conds, None, [F.sum(Col("l_extendedprice") * Col("l_discount"))])
    yield agg_case("scalar_for16_both_orders", "scalar", _cols_of(low, kinds, _dummy()), low)
    # ---- the opcodes across the forms: the lowering's CASE and date-part programs, then every opcode by hand
    ts = Col("ts")
    urgent = (Col("d") == "apple") | Col("d").like("b%")
    sel = [F.sum(F.when(urgent, 1).otherwise(0)), F.sum(F.when(Col("b") > 0, Col("f")).otherwise(0)),
           F.max(F.when(Col("s") == "x", Col("a")).when(Col("a") > 3, Col("b")).otherwise(Col("f"))), F.sum(F.when(Lit(0), 5).otherwise(7))]
    part = [F.sum(F.when(F.year(ts) == 1996, Col("f")).otherwise(0)), F.max(F.quarter(ts) * 10 + F.dayofweek(ts)),
            F.min(F.dayofyear(F.date_trunc("week", ts))), F.sum(F.year(Lit(datetime(2024, 2, 29)))),
            F.max(F.day(F.date_trunc("month", F.date_trunc("year", Col("t2")))))]
    for name, where, what in (("sel", [F.when(Col("a") > 0, Col("a")).otherwise(Col("b")) > Lit(5)], sel),
                              ("datepart", [(F.month(ts) == 2) & (F.day(ts) == 29)], part)):
        for entry in ("private", "shared", "scalar"):
            low = lower_aggregate(SCHEMA, KINDS, where, None if entry == "scalar" else Col("a"), what, DICTS)
            yield agg_case(f"{entry}_{name}", entry, _hs_cols(low.program, KINDS), low)
    b = ProgramBuilder(SCHEMA, KINDS, DICTS)
    b.emit_out(0, F.when(Col("a") > Col("b"), Col("f")).otherwise(0))
    b.emit_out(1, Lit(1) + F.when(Col("s").like("x%"), Col("a")).when(urgent, 2).otherwise(Col("b")))
    b.emit_out(2, F.when(Lit(0), 5).otherwise(7))
    b.emit_out(3, F.year(ts) * 100 + F.month(F.date_trunc("quarter", Col("t2"))))
    b.emit_out(4, F.year(Lit(datetime(2024, 2, 29))))
    b.emit_out(5, F.date_trunc("minute", ts) == F.date_trunc("second", Col("t2")))
    program = b.finish()
    yield ("eval_sel_datepart", "eval", _hs_cols(program, KINDS), len(program.columns), program.to_struct(),
           (C.c_int32 * 6)(hs.F64, hs.I64, hs.I64, hs.I64, hs.I64, hs.U8), -1, -1, 6)
    exprs = jp.expressions()
    for entry in jp.ENTRY_POINTS:
        prog, tail = jp.out_program(exprs) if entry == "eval" else jp.agg_program(entry != "scalar", exprs)
        kinds_out = (C.c_int32 * hs.HS_MAX_OUTS)(*[hs.U8 if i % 2 else hs.F64 for i in range(hs.HS_MAX_OUTS)])
        yield (f"{entry}_every_opcode", entry, jp.columns(), len(jp.COLUMN_KINDS), prog, kinds_out if entry == "eval" else tail,
               -1 if entry in ("scalar", "eval") else jp.A, -1, tail if entry == "eval" else 0)
    for entry in ("private", "shared", "scalar"):
        prog, spec = jp.agg_program(entry != "scalar", [jp.DICTBIT_NOT_PRELOADED])
        yield f"{entry}_dictbit_not_preloaded", entry, jp.columns(), len(jp.COLUMN_KINDS), prog, spec, -1 if entry == "scalar" else jp.A, -1, 0
    # ---- hs_eval: every plain input kind, one-byte and 8-byte outputs, several outputs
    kinds_in = [hs.I32, hs.F32, hs.I64, hs.F64, hs.U8]
    words = [x for slot in range(5) for x in (w(op.OP_LD, 0, slot), w(op.OP_OUT, 1, slot))]
    yield ("eval_every_input_kind", "eval", jp.columns(kinds_in), 5, jp.program(words),
           (C.c_int32 * 5)(hs.I64, hs.F64, hs.I64, hs.F64, hs.U8), -1, -1, 5)
    from tests.test_abi import eval_program

    program, kinds_e, out_kinds = eval_program()
    cols = (hs.hs_col * len(program.columns))()
    for slot, idx in enumerate(program.columns):
        cols[slot].kind, cols[slot].fixed_len = kinds_e[idx], -1
    yield "eval_abi_expressions", "eval", cols, len(program.columns), program.to_struct(), out_kinds, -1, -1, len(out_kinds)
    # ---- declined programs: one per text
    for i, (what, (words, _why)) in enumerate(jp.DECLINED.items()):
        for entry in jp.ENTRY_POINTS:
            lead = [w(op.OP_KEY, 0)] if entry in ("private", "shared") else []
            yield _raw(f"declined_{entry}_{i}_" + what.replace(" ", "_"), entry, jp.COLUMN_KINDS, lead + words)
    ld_agg = [w(op.OP_LD, 0, 1), w(op.OP_AGG, 1, 0)]
    key = w(op.OP_KEY, 0)
    yield _raw("declined_narrow_in_the_shared_tier", "shared", [hs.I32, hs.I64_FOR16], [key] + ld_agg)
    yield _raw("declined_narrow_key", "private", [hs.I64_FOR16, hs.F32], [key] + ld_agg)
    yield _raw("declined_lut_without_entries", "private", [hs.I32, hs.F32_LUT8], [key] + ld_agg, fixed={1: 0})
    yield _raw("declined_pair_in_the_private_tier", "private", [hs.I32, hs.PAIR | hs.F32], [key] + ld_agg)
    yield _raw("declined_pair_key", "shared", [hs.PAIR | hs.I32, hs.F32], [key] + ld_agg)
    yield _raw("declined_pair_read_as_a_string", "shared", [hs.I32, hs.PAIR | hs.I32],
               [key, w(op.OP_DICTBIT, 0, 1, 0, 1), w(op.OP_AGG, 1, 0)])
    yield _raw("declined_unknown_column_kind", "private", [hs.I32, 99], [key] + ld_agg)
    yield _raw("declined_join8_without_its_unit", "shared", [hs.JOIN8_CODE, hs.F32, hs.JOIN8_UNIT], [key] + ld_agg, fixed={0: 1})
    yield _raw("declined_ld_of_a_string", "private", [hs.I32, hs.STR], [key] + ld_agg)
    yield _raw("declined_key_in_a_keyless_program", "scalar", [hs.I32, hs.F32], [key] + ld_agg)
    yield _raw("declined_unit_column_not_a_byte", "shared", [hs.I32, hs.F32], [key] + ld_agg, unit=1)
    yield _raw("declined_agg_before_key", "private", [hs.I32, hs.F32], ld_agg + [key])
    yield _raw("declined_bad_accumulator", "private", [hs.I32, hs.F32], [key, w(op.OP_LD, 0, 1), w(op.OP_AGG, 1, 5)])
    yield _raw("declined_accumulator_fed_twice", "private", [hs.I32, hs.F32], [key] + ld_agg + ld_agg)
    for entry in ("private", "shared"):
        yield _raw(f"declined_{entry}_aggregates_without_a_key", entry, [hs.I32, hs.F32], [], n_acc=1)
    for entry in ("shared", "scalar"):
        yield _raw(f"declined_{entry}_accumulator_never_fed", entry, [hs.I32, hs.F32], [key] * (entry == "shared") + ld_agg, n_acc=2)
    yield _raw("declined_eval_ld_of_a_string", "eval", [hs.I32, hs.STR], [w(op.OP_LD, 0, 1), w(op.OP_OUT, 1, 0)])
    yield _raw("declined_eval_ld_of_a_missing_column", "eval", [hs.I32], [w(op.OP_LD, 0, 3), w(op.OP_OUT, 1, 0)])
    yield _raw("declined_eval_unknown_column_kind", "eval", [hs.I32, hs.I64_FOR16], [w(op.OP_LD, 0, 1), w(op.OP_OUT, 1, 0)])
    yield _raw("declined_eval_out_written_twice", "eval", [hs.I32], [w(op.OP_LD, 0, 0), w(op.OP_OUT, 1, 0)] * 2)
    yield _raw("declined_eval_out_beyond_the_outputs", "eval", [hs.I32], [w(op.OP_LD, 0, 0), w(op.OP_OUT, 1, hs.HS_MAX_OUTS)])


def generate(lib, case):
    """-> (return code, source text): one corpus entry through its hs_jit_compile_check* entry point."""
    _name, entry, cols, n_cols, prog, tail, key, unit, n_outs = case
    rc, text, _size = jp.compile_check(lib, entry, cols, n_cols, prog, tail, key=key, unit=unit, n_outs=n_outs)
    return rc, text


def write_corpus(folder: Path) -> int:
    lib = hs.load_library()
    folder.mkdir(parents=True, exist_ok=True)
    lines, failed = [], 0
    for case in corpus():
        rc, text = generate(lib, case)
        if rc == 0:
            (folder / f"{case[0]}.hip").write_text(text)
            lines.append(f"{case[0]} {hashlib.sha256(text.encode()).hexdigest()}")
        elif rc == 2 and case[0].startswith("declined_"):
            lines.append(f"{case[0]} DECLINED: {lib.hs_last_error().decode()}")
        else:  # a program the corpus expects to compile did not: say so and fail
            failed += 1
            lines.append(f"{case[0]} FAILED rc={rc}: {lib.hs_last_error().decode()}")
    (folder / "MANIFEST").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return failed


def main(argv) -> int:
    if "--corpus" in argv:
        return 1 if write_corpus(Path(argv[argv.index("--corpus") + 1])) else 0
    lib = hs.load_library()
    if "--join" in argv:
        cols, n, low = join8()
        case = agg_case("join", "shared", cols, low, n, unit=n - 1)
    else:
        cols, low = q1("--narrow" in argv)
        case = agg_case("q1", "private", cols, low)
    rc, text = generate(lib, case)
    print(text)
    if rc:
        raise SystemExit(lib.hs_last_error().decode() + "\n" + lib.hs_jit_last_log().decode()[:4000])
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
