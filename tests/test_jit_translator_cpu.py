"""The run-time compiler's one translator (csrc/hs_jit.hip, Translator) without a GPU: what the aggregate generator compiles
the expression generator compiles too, and what one declines the other declines with the same words.  The programs are
tests/jit_programs.py's; the opcode list is read from minispark_amd.hipspark, so an opcode added there and not covered
here - or covered by one generator only - fails."""

from __future__ import annotations

import pytest

from minispark_amd import hipspark as hs
from tests import jit_programs as jp


def test_the_programs_hold_every_expression_opcode_within_the_limits():
    exprs = jp.expressions()
    held = set().union(*(jp.opcodes_of(e) for e in exprs))
    missing = {name for name, value in jp.EXPRESSION_OPS.items() if value not in held}
    assert not missing, f"opcodes without a program in tests/jit_programs.py: {sorted(missing)}"
    assert held == set(jp.EXPRESSION_OPS.values())
    # one program per form: the limits of a program are not what splits them
    assert len(exprs) <= min(hs.HS_MAX_OUTS, hs.HS_MAX_ACC)
    assert sum(len(e) + 1 for e in exprs) + 1 <= hs.HS_MAX_INS
    for e in exprs:
        assert max((w >> 8) & 0xFF for w in e) + 1 <= hs.HS_MAX_STACK


@pytest.mark.parametrize("entry", jp.ENTRY_POINTS)
def test_every_expression_opcode_compiles_behind_out_and_behind_agg(entry):
    """OUT through hs_jit_compile_check_eval; AGG through _scalar, and with a key through hs_jit_compile_check and _shared."""
    lib = hs.load_library()
    exprs = jp.expressions()
    rc, text, size = jp.check_expressions(lib, entry, exprs)
    assert rc == 0, (entry, lib.hs_last_error(), lib.hs_jit_last_log()[:2000])
    assert size > 1000
    n = lambda op: sum(1 for e in exprs for w in e if (w & 0xFF) == op)  # noqa: E731
    binary = sum(1 for e in exprs for w in e if hs.OP_ADD_F <= (w & 0xFF) <= hs.OP_OR)
    assert text.count("hs_bin<") == binary >= 25  # every operator once; ADD_F and OR also join the other opcodes' values
    for op in range(hs.OP_ADD_F, hs.OP_OR + 1):
        assert f"hs_bin<{op}>(" in text
    assert text.count("(double)(long long)") == n(hs.OP_I2F) == 4
    assert text.count(" != 0 ? ") == n(hs.OP_SEL) == 2 and text.count("hs_datepart_c<") == n(hs.OP_DATEPART) == 2
    assert text.count("hs_strcmp_lit(") == 1 and text.count("hs_strcmp_col(") == 1 and text.count("hs_like_lit(") == 1
    assert text.count("hs_dictbit") == 1
    # the aggregate forms define a row-invariant value once, ahead of the row loop; hs_eval's kernel per row
    head = text.partition("for (int j = 0; j < ")[0]
    hoisted = [line for line in head.splitlines() if line.strip().startswith("const unsigned long long k")]
    if entry == "eval":
        assert not hoisted and "hs_dictbit(" in text
    else:
        assert sum("hs_datepart_c<19u>(k" in line for line in hoisted) == 1 and sum(" != 0 ? k" in line for line in hoisted) == 1
        assert sum("(double)(long long)k" in line for line in hoisted) == 2 and "hs_dictbit_code(" in text


@pytest.mark.parametrize("what", list(jp.DECLINED))
def test_all_four_entry_points_decline_with_the_same_words(what):
    lib = hs.load_library()
    words, why = jp.DECLINED[what]
    said = {}
    for entry in jp.ENTRY_POINTS:
        rc, _text, _size = jp.check_expressions(lib, entry, words, whole=True)
        assert rc == 2, (entry, rc, lib.hs_last_error())  # HS_E_LIMIT: declined, not an error of the call
        said[entry] = lib.hs_last_error().decode().partition(": ")[2]
    assert set(said.values()) == {why}, said
