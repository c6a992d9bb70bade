"""tests/agg_scan_model.py pinned without a GPU: the edge table written as a BlockFile with the units as blocks, the
equivalent ``filter(keep == 1).group_by(k).agg(...)`` run through the oracle.  The model's per-unit rows, merged by
agg_tail_models.fold_partials and stored again, are the oracle's result rows for the quiet scenarios; every raising scenario
makes the oracle raise the exception its flag stands for; and the conditions the GPU comparison rests on (no skipped cell,
exact sums - build_table asserts those itself) hold for every launch the GPU tests make."""

from __future__ import annotations

import struct

import pytest

from minispark_amd import hipspark as hs
from tests import agg_scan_model as m
from tests.agg_tail_models import fold_partials, store


def _frame(engine, path, program):
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col

    return DataFrame(engine).table(str(path)).filter(Col("keep") == 1).group_by(Col("k")).agg(*program.aggs)


def _write(table, path):
    from minispark_amd.io import BlockFile

    BlockFile(path).write_raw_blocks(m.SCHEMA, table.blocks())


def _value(token, kind):
    if token == "nan":
        return float("nan")
    data = struct.pack("<I", token)
    return struct.unpack("<f", data)[0] if kind == hs.F32 else int.from_bytes(data, "little", signed=True)


def _row_tokens(rows, program):
    out = {}
    for row in rows:
        cells = []
        for name, kind in zip(program.names, program.kinds):
            data, raised = store(row[name], kind)
            assert raised == 0
            cells.append(m.cell_token(data, kind))
        assert row["k"] not in out
        out[row["k"]] = tuple(cells)
    return out


@pytest.mark.parametrize("program", ["six", "quot"])
def test_merged_model_rows_are_the_oracles_rows_for_the_quiet_scenarios(tmp_path, program):
    from oracle.py_engine import run_query

    scenarios, filler, live = m.LAUNCHES["wide"][0]
    table, units, flags = m.expected(scenarios, filler, live, program, False, False)  # one copy: the units are merged
    prog = m.programs()[program]
    assert flags == 0 and not m.undefined_cells(units)
    assert len(units[m.LONG_UNIT]) == len(scenarios) + len(filler)
    partials = [(u, j, key, [_value(t, kind) for t, kind in zip(cells, prog.kinds)])
                for u, unit in enumerate(units) for j, (key, cells) in enumerate(unit.items())]
    merged = fold_partials(partials, list(enumerate(prog.ops)))
    want = {}
    for key, values in merged.items():
        cells = [store(v, kind) for v, kind in zip(values, prog.kinds)]
        assert all(raised == 0 for _, raised in cells)
        want[key] = tuple(m.cell_token(data, kind) for (data, _), kind in zip(cells, prog.kinds))
    _write(table, tmp_path / "t.bin")
    got = _row_tokens(run_query(_frame(object(), tmp_path / "t.bin", prog).task), prog)
    assert got == want


@pytest.mark.parametrize(("scenario", "program"), [(s.name, entry[0]) for s in m.RAISING for entry in s.raising])
def test_the_oracle_raises_what_the_flag_stands_for(tmp_path, scenario, program):
    from oracle.py_engine import run_query

    flag, exception, aggs = m.SCENARIOS[scenario].raises_in(program)
    table, units, flags = m.expected((scenario,), m.FILLER_KEYS[:1], True, program, False, False)
    prog = m.programs()[program]
    assert flags == flag
    assert m.undefined_cells(units) == {(m.LONG_UNIT, m.SCENARIO_KEY[scenario], prog.names.index(a)) for a in aggs}
    _write(table, tmp_path / "t.bin")
    with pytest.raises(exception):
        run_query(_frame(object(), tmp_path / "t.bin", prog).task)


@pytest.mark.parametrize("shape", ["wide", "narrow", "keyless"])
def test_every_launch_skips_only_the_raising_cells(shape):
    """Per launch of the GPU tests, on the "six" program (the "quot" launches of the wide shape are covered above): flags
    and None cells are exactly the raising scenarios', and every copy of a group gives the cells of its long-unit copy."""
    keyless = shape == "keyless"
    prog = m.programs()["six"]
    launches = m.LAUNCHES[shape] if shape != "narrow" else m.LAUNCHES[shape][:5]  # (the raising ones: as "wide", one filler key)
    for scenarios, filler, live in launches:
        table, units, flags = m.expected(scenarios, filler, live, "six", keyless)
        assert flags == m.expected_flags(table, prog), scenarios
        assert m.undefined_cells(units) == m.expected_undefined(table, prog, keyless), scenarios
        if not any(m.SCENARIOS[s].raising for s in scenarios):
            assert flags == 0 and not m.undefined_cells(units)
        for name in scenarios if not keyless else ():
            key = m.SCENARIO_KEY[name]
            assert len(table.placed[name]) == 2, f"{name} found no small unit"
            for u in table.placed[name]:
                assert units[u][key] == units[m.LONG_UNIT][key], (name, u)


def test_edge_rows_sit_where_the_kernels_change_hands():
    scenarios, filler, live = m.LAUNCHES["wide"][0]
    table = m.build_table(scenarios, filler, live)
    k = table.columns["k"]
    base = m.BOUNDS[m.LONG_UNIT]
    for row in (0, 3, 4, 1023, 1024, 1025, 65535, 65536, 65537, m.UNIT_SIZES[m.LONG_UNIT] - 1):
        assert k[base + row] >= 100, row
    for u in range(1, m.LONG_UNIT):  # first and last row of every small unit that can hold a scenario
        assert k[m.BOUNDS[u]] >= 100 and k[m.BOUNDS[u + 1] - 1] >= 100, u
    for name in scenarios:  # every group of the long unit has live rows in both 65 536-row chunks
        rows = (k[base:] == m.SCENARIO_KEY[name]).nonzero()[0]
        assert rows.min() < 65536 <= rows.max(), name
