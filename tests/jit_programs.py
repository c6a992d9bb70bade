"""Hand-built bytecode for the run-time compiler's translator (csrc/hs_jit.hip), shared by tests/test_jit_translator_cpu.py
and the corpus of tools/jit_source.py: one program that holds every expression opcode, and the malformed programs every
generator declines.  The opcode list is read from minispark_amd.hipspark: a new opcode lands in EXPRESSION_OPS by itself."""

from __future__ import annotations

import ctypes as C

from minispark_amd import hipspark as hs

SINKS = {"OP_END", "OP_FILTER", "OP_KEY", "OP_AGG", "OP_OUT"}  # what is not an expression opcode
EXPRESSION_OPS = {name: value for name, value in vars(hs).items()
                  if name.startswith("OP_") and isinstance(value, int) and name not in SINKS}

# the column table the programs below are written against
A, F, T, S, S2, D = range(6)  # INTEGER (also the key of the keyed forms), FLOAT, TIMESTAMP, two STRINGs, a code byte
COLUMN_KINDS = [hs.I32, hs.F32, hs.I64, hs.STR, hs.STR, hs.U8]


def word(op: int, sp: int, a: int = 0, b: int = 0, c: int = 0) -> int:
    return op | (sp << 8) | (a << 16) | (b << 32) | (c << 48)


def columns(kinds=COLUMN_KINDS):
    cols = (hs.hs_col * len(kinds))()
    for slot, kind in enumerate(kinds):
        cols[slot].kind, cols[slot].fixed_len = kind, -1
    return cols


def program(words) -> hs.hs_program:
    p = hs.hs_program()
    p.n_ins, p.n_lit = len(words), 4
    for i, w in enumerate(words):
        p.ins[i] = w
    return p


def spec(n_acc: int) -> hs.hs_agg_spec:
    s = hs.hs_agg_spec()
    s.n_acc = n_acc  # every accumulator a float SUM
    return s


def _chain(first: int, ops, operand) -> list[int]:
    """column `first`, then `operand` and one binary operator per entry of `ops`: a left-deep chain, depth 2."""
    words = [word(hs.OP_LD, 0, first)]
    for op in ops:
        words += [operand(1), word(op, 2)]
    return words


def expressions() -> list[list[int]]:
    """Expressions (each leaves one cell on an empty stack) that together hold every opcode of EXPRESSION_OPS."""
    lit = lambda sp: word(hs.OP_LIT, sp, 0)  # noqa: E731
    ld_a = lambda sp: word(hs.OP_LD, sp, A)  # noqa: E731
    return [
        _chain(F, range(hs.OP_ADD_F, hs.OP_MOD_F + 1), lit),
        _chain(A, range(hs.OP_ADD_I, hs.OP_MOD_I + 1), ld_a),
        _chain(F, range(hs.OP_LT_F, hs.OP_NE_F + 1), lit),
        _chain(A, range(hs.OP_LT_I, hs.OP_OR + 1), ld_a),
        # I2F of the top cell (a row value, a literal) and of the cell below it (a row value, a literal)
        [word(hs.OP_LD, 0, A), word(hs.OP_I2F, 1, 0), word(hs.OP_LIT, 1, 1), word(hs.OP_I2F, 2, 0), word(hs.OP_ADD_F, 2),
         word(hs.OP_LD, 1, A), word(hs.OP_LD, 2, F), word(hs.OP_I2F, 3, 1), word(hs.OP_ADD_F, 3), word(hs.OP_ADD_F, 2),
         word(hs.OP_LIT, 1, 1), word(hs.OP_LD, 2, F), word(hs.OP_I2F, 3, 1), word(hs.OP_ADD_F, 3), word(hs.OP_ADD_F, 2)],
        [word(hs.OP_STRCMP_LIT, 0, S, 2, 4), word(hs.OP_STRCMP_COL, 1, S, S2, 5), word(hs.OP_OR, 2),
         word(hs.OP_LIKE, 1, S2, 3), word(hs.OP_OR, 2), word(hs.OP_DICTBIT, 1, D, 0, 1), word(hs.OP_OR, 2)],
        # CASE and a date part on row values, then on literals only (row-invariant: the aggregate forms hoist them)
        [word(hs.OP_LD, 0, A), word(hs.OP_LD, 1, T), word(hs.OP_DATEPART, 2, 0), word(hs.OP_LIT, 2, 0), word(hs.OP_SEL, 3)],
        [word(hs.OP_LIT, 0, 0), word(hs.OP_LIT, 1, 1), word(hs.OP_DATEPART, 2, 19), word(hs.OP_LIT, 2, 0), word(hs.OP_SEL, 3)],
    ]


DICTBIT_NOT_PRELOADED = [word(hs.OP_DICTBIT, 0, S, 0, 1)]  # the code read from memory (the aggregate forms' other arm)


def opcodes_of(words) -> set[int]:
    return {w & 0xFF for w in words}


def out_program(exprs=None) -> tuple[hs.hs_program, int]:
    """-> (program, outputs): expression i is output i (hs_eval's form)."""
    exprs = expressions() if exprs is None else exprs
    words = [w for i, e in enumerate(exprs) for w in [*e, word(hs.OP_OUT, 1, i)]]
    return program(words), len(exprs)


def agg_program(keyed: bool, exprs=None) -> tuple[hs.hs_program, hs.hs_agg_spec]:
    """-> (program, spec): expression i feeds accumulator i, behind HS_OP_KEY for the keyed tiers."""
    exprs = expressions() if exprs is None else exprs
    words = ([word(hs.OP_KEY, 0)] if keyed else []) + [w for i, e in enumerate(exprs) for w in [*e, word(hs.OP_AGG, 1, i)]]
    return program(words), spec(len(exprs))


# malformed expressions: what every generator must decline, and the text it declines with
DECLINED = {
    "a wrong depth annotation": ([word(hs.OP_LD, 1, A)], "stack depth annotation does not match"),
    "an underflow on a binary operator": ([word(hs.OP_ADD_I, 0)], "stack underflow"),
    "an underflow on SEL": ([word(hs.OP_SEL, 0)], "stack underflow"),
    "an underflow on DATEPART": ([word(hs.OP_DATEPART, 0, 0)], "stack underflow"),
    "an unbalanced program": ([word(hs.OP_LD, 0, A)], "unbalanced program"),
    "an unknown opcode": ([word(200, 0)], "opcode not covered by the translator"),
    "a DATEPART selector out of range": ([word(hs.OP_LD, 0, T), word(hs.OP_DATEPART, 1, 9)], "DATEPART selector out of range"),
}

ENTRY_POINTS = ("private", "shared", "scalar", "eval")


def compile_check(lib, entry: str, cols, n_cols: int, prog, spec_or_kinds, key: int = -1, unit: int = -1, n_outs: int = 0,
                  cap: int = 1 << 17) -> tuple[int, str, int]:
    """One hs_jit_compile_check* call -> (return code, generated source, code-object bytes)."""
    src, size = C.create_string_buffer(cap), C.c_int64(0)
    if entry == "eval":
        rc = lib.hs_jit_compile_check_eval(cols, n_cols, C.byref(prog), spec_or_kinds, n_outs, b"gfx950", C.byref(size), src, cap)
    elif entry == "scalar":
        rc = lib.hs_jit_compile_check_scalar(cols, n_cols, C.byref(prog), C.byref(spec_or_kinds), b"gfx950", C.byref(size), src, cap)
    elif entry == "shared":
        rc = lib.hs_jit_compile_check_shared(cols, n_cols, key, unit, C.byref(prog), C.byref(spec_or_kinds), b"gfx950",
                                             C.byref(size), src, cap)
    else:
        rc = lib.hs_jit_compile_check(cols, n_cols, key, C.byref(prog), C.byref(spec_or_kinds), b"gfx950", C.byref(size), src, cap)
    return rc, src.value.decode(), size.value


def check_expressions(lib, entry: str, words_or_exprs, whole: bool = False) -> tuple[int, str, int]:
    """The expressions (or, `whole`, one malformed run of words) through one entry point over COLUMN_KINDS."""
    cols, n = columns(), len(COLUMN_KINDS)
    if entry == "eval":
        prog, n_outs = (program(words_or_exprs), 1) if whole else out_program(words_or_exprs)
        kinds = (C.c_int32 * hs.HS_MAX_OUTS)(*[hs.U8 if i % 2 else hs.F64 for i in range(hs.HS_MAX_OUTS)])
        return compile_check(lib, entry, cols, n, prog, kinds, n_outs=n_outs)
    keyed = entry != "scalar"
    if whole:
        prog, sp = program(([word(hs.OP_KEY, 0)] if keyed else []) + list(words_or_exprs)), spec(1)
    else:
        prog, sp = agg_program(keyed, words_or_exprs)
    return compile_check(lib, entry, cols, n, prog, sp, key=A if keyed else -1)
