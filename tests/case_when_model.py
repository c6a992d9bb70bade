"""CPU model of CASE WHEN for the tests: the oracle's ``compile_expr`` with one more node class.

The oracle (oracle/py_engine.py) dispatches on class names and does not know ``CaseColumn`` - the reference has no CASE.
``compile_expr`` below handles that class and hands every other node to the oracle's own function.  The oracle's
recursion and its filter / project / aggregate helpers look ``compile_expr`` up in their module at call time, so with

    monkeypatch.setattr(oracle.py_engine, "compile_expr", case_when_model.compile_expr)

nested and aggregated CASEs go through the model too, and the oracle's quantisation points, per-block partial sums and
merge order apply unchanged.

Semantics: the condition and BOTH branches are evaluated for the row - whatever a branch raises is
raised, taken or not - then the chosen value is returned, through ``float()`` when the CASE is FLOAT-valued (either
branch FLOAT), as the device converts the INTEGER branch with I2F.
"""

from __future__ import annotations

from typing import Any, Callable

import oracle.py_engine as py_engine

_oracle_compile_expr = py_engine.compile_expr  # the oracle's own, bound before any test patches the module


def compile_expr(expr: Any, schema: list[tuple[str, Any]]) -> Callable[[tuple], Any]:
    if type(expr).__name__ != "CaseColumn":
        return _oracle_compile_expr(expr, schema)
    cond = py_engine.compile_expr(expr.condition, schema)  # looked up at call time: this function while installed
    then = py_engine.compile_expr(expr.then_col, schema)
    other = py_engine.compile_expr(expr.else_col, schema)
    is_float = getattr(expr.infer_type(list(schema)), "name", None) == "FLOAT"

    def run(row: tuple) -> Any:
        c, x, y = cond(row), then(row), other(row)  # eager: all three, then the choice
        value = x if c else y
        return float(value) if is_float else value

    return run


def install(monkeypatch: Any) -> None:
    """For the duration of the test: the oracle evaluates CaseColumn through the model."""
    monkeypatch.setattr(py_engine, "compile_expr", compile_expr)
