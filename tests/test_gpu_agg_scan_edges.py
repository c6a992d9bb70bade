"""Every partial-aggregate scan against tests/agg_scan_model.py at the values where a fold or an atomic goes wrong: NaN next
to MIN / MAX, infinities, the int identities a FLOAT MIN / MAX must not keep, the f32 overflow boundary of a SUM, f32
denormals through the f64 -> f32 store, and rows that failed the WHERE clause.  One harness calls the tier at the Device
level, cuts the partial rows by unit and compares them with the model as a set of (key -> stored bits) per unit, and the
status word with the model's flags - no tolerance (the data makes every order of additions exact; a NaN is compared as
"is NaN"), and no cell skipped but the ones the reference has no bytes for.  On top, the same tables as whole queries with
the short tail on and off."""

from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

from tests import agg_scan_model as m

pytestmark = pytest.mark.gpu

N_UNITS = len(m.UNIT_SIZES)


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


def _upload(dev, table):
    return [dev.upload_raw(table.columns[name], col_type) for name, col_type in m.SCHEMA]


def _unit_col(dev, table):
    """Computed units: the unit id of every row, 0xff (dropped) where keep = 0."""
    import torch

    unit = np.repeat(np.arange(N_UNITS, dtype=np.uint8), m.UNIT_SIZES)
    unit[table.columns["keep"] == 0] = 0xFF
    return dev.to_device(unit, torch.uint8)


def _bits(col, n):
    return col.data[:n].cpu().numpy().view(np.uint32).tolist()


def _cut(keys, cells, unit_of_row, kinds, keyless):
    """Downloaded partial rows -> [{key: cell tokens} per unit]; a key twice in one unit is an error of its own."""
    units = [{} for _ in range(N_UNITS)]
    for r, u in enumerate(unit_of_row):
        key = 0 if keyless else keys[r]
        assert key not in units[u], f"unit {u} emitted key {key} twice"
        units[u][key] = tuple(m.cell_token(struct.pack("<I", col[r]), kind) for col, kind in zip(cells, kinds))
    return units


def _run(dev, tier, table, prog):
    """One launch of `tier` over the table -> ([{key: cell tokens} per unit], flags)."""
    from minispark_amd.device import DBatch
    from minispark_amd.sql import Col

    cols, units_ids = _upload(dev, table), list(range(N_UNITS))
    keyless = tier == "keyless"
    dev.reset_flags()
    if tier in ("radix", "hash"):
        batch = DBatch(list(m.SCHEMA), cols, m.N_ROWS, list(m.BOUNDS))
        dev.radix_enabled = tier == "radix"
        try:
            out = dev.aggregate_partial_global(batch, prog.filters, Col("k"), list(prog.aggs), prog.out_schema)
        finally:
            dev.radix_enabled = True
        assert dev.last_global_tier == tier
        n = out.nrows
        unit_of_row = np.repeat(np.arange(N_UNITS), np.diff(out.unit_rows)).tolist()
        assert len(unit_of_row) == n
    else:
        if tier == "units":
            batch = DBatch(list(m.SCHEMA), cols, m.N_ROWS, unit_ids=units_ids, unit_col=_unit_col(dev, table), n_unit_ids=N_UNITS)
            out = dev.aggregate_partial(batch, [], Col("k"), list(prog.aggs), prog.out_schema, group_cap_hint=512, shared=True)
            assert dev.last_scan["chunks"] > 1  # (one row range: its 70 464 rows are more than one chunk)
        else:
            batch = DBatch(list(m.SCHEMA), cols, m.N_ROWS, list(m.BOUNDS), unit_ids=units_ids)
            out = dev.aggregate_partial(batch, prog.filters, None if keyless else Col("k"), list(prog.aggs), prog.out_schema,
                                        group_cap_hint={"private": 4, "shared": 64, "keyless": 1}[tier], shared=tier == "shared")
            assert dev.last_scan["chunks"] > N_UNITS, "the long unit must span several workgroups"
        assert dev.last_scan["tier"] == {"private": "private", "shared": "shared", "units": "shared", "keyless": "scalar"}[tier]
        n = int(out.nrows_dev[0].item()) if out.nrows_dev is not None else out.nrows
        unit_of_row = out.order[:n].cpu().tolist()
    keys = out.cols[0].data[:n].cpu().tolist()
    cells = [_bits(col, n) for col in out.cols[1:]]
    flags = dev.read_flags()
    dev.reset_flags()
    return _cut(keys, cells, unit_of_row, prog.kinds, keyless), flags


def _compare(dev, tier, table, prog, want, want_flags, where):
    got, flags = _run(dev, tier, table, prog)
    assert flags == want_flags, f"{where}: flags {flags:#x}, the model's {want_flags:#x}"
    for u, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), f"{where}: unit {u} holds keys {sorted(g)}, the model's {sorted(w)}"
        for key, cells in w.items():
            for a, (have, cell) in enumerate(zip(g[key], cells)):
                assert cell is None or have == cell, f"{where}: unit {u} key {key} {prog.names[a]}: {have!r}, the model's {cell!r}"


def _check(dev, tier, shape, program):
    prog = m.programs()[program]
    for scenarios, filler, live in m.LAUNCHES[shape]:
        table, want, want_flags = m.expected(scenarios, filler, live, program, tier == "keyless")
        assert m.undefined_cells(want) == m.expected_undefined(table, prog, tier == "keyless"), scenarios
        _compare(dev, tier, table, prog, want, want_flags, f"{tier} {program} {scenarios}")


class _Form:
    """Compiled (jit) or interpreted form for the launches inside; the way out restores the compiled form and checks
    hs_jit_stats: launches of run-time compiled kernels happened exactly when the compiled form was asked for."""

    def __init__(self, dev, jit: bool) -> None:
        self.lib, self.jit, self.stats = dev.lib, jit, (C.c_int32 * 3)()

    def __enter__(self):
        self.lib.hs_jit_stats(self.stats)
        self.before = self.stats[1]
        self.lib.hs_jit_set_enabled(1 if self.jit else 0)
        return self

    def __exit__(self, exc_type, *_):
        self.lib.hs_jit_set_enabled(1)
        self.lib.hs_jit_stats(self.stats)
        if exc_type is None:
            assert (self.stats[1] > self.before) == self.jit, "the compiled / interpreted form was not the one exercised"


@pytest.mark.parametrize("program", ["six", "quot"])
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreted"])
def test_private_table_scan(dev, jit, program):
    with _Form(dev, jit):
        _check(dev, "private", "narrow", program)


@pytest.mark.parametrize("program", ["six", "quot"])
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreted"])
def test_shared_dictionary_scan(dev, jit, program):
    with _Form(dev, jit):
        _check(dev, "shared", "wide", program)


@pytest.mark.parametrize("program", ["six", "quot"])
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreted"])
def test_shared_scan_with_computed_units(dev, jit, program):
    with _Form(dev, jit):
        _check(dev, "units", "wide", program)


@pytest.mark.parametrize("program", ["six", "quot"])
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreted"])
def test_keyless_scan(dev, jit, program):
    with _Form(dev, jit):
        _check(dev, "keyless", "keyless", program)


@pytest.mark.parametrize("program", ["six", "quot"])
@pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreted"])
@pytest.mark.parametrize("tier", ["radix", "hash"])
def test_hbm_tiers(dev, tier, jit, program):
    """(Both HBM tiers evaluate the WHERE over whole columns - compiled or interpreted, which is what the launch counter
    sees here - and the aggregate arguments over the surviving rows' list, which hs_eval only interprets.)"""
    with _Form(dev, jit):
        _check(dev, tier, "wide", program)


@pytest.mark.parametrize("tier", ["private", "shared", "units", "keyless", "radix", "hash"])
def test_one_changed_row_is_noticed_on_every_tier(dev, tier):
    """The comparison itself: the model's answer for the table as built, the tier run over a table with ONE row changed -
    a dead NaN row brought to life (its group's SUM turns NaN), then 2^102 more in the SUM that just rounded down to FLT_MAX
    (it overflows: a flag and no other difference)."""
    import copy

    scenarios, filler, live = {"private": m.LAUNCHES["narrow"][4], "keyless": m.LAUNCHES["keyless"][14]}.get(tier, m.LAUNCHES["wide"][0])
    prog = m.programs()["six"]
    table, want, want_flags = m.expected(scenarios, filler, live, "six", tier == "keyless")
    changed = copy.deepcopy(table)
    k, f = changed.columns["k"], changed.columns["f"]
    row = int(((k == m.SCENARIO_KEY["dead_rows_hold_the_edges"]) & np.isnan(f)).nonzero()[0][0])
    assert changed.columns["keep"][row] == 0
    changed.columns["keep"][row] = 1
    with pytest.raises(AssertionError, match="sf: 'nan'"):
        _compare(dev, tier, changed, prog, want, want_flags, tier)
    scenarios, filler, live = {"private": m.LAUNCHES["narrow"][2], "keyless": m.LAUNCHES["keyless"][8]}.get(tier, m.LAUNCHES["wide"][0])
    table, want, want_flags = m.expected(scenarios, filler, live, "six", tier == "keyless")
    changed = copy.deepcopy(table)
    row = int((changed.columns["f"] == np.float32(-(2.0**102))).nonzero()[0][0])
    changed.columns["f"][row] = 0.0
    with pytest.raises(AssertionError, match="flags 0x4, the model's 0x0"):
        _compare(dev, tier, changed, prog, want, want_flags, tier)


# ---- whole queries: the same tables through the engine, short tail on and off ---------------------------------------
def _frame(engine, path, prog):
    from minispark_amd.dataframe import DataFrame
    from minispark_amd.sql import Col

    return DataFrame(engine).table(str(path)).filter(Col("keep") == 1).group_by(Col("k")).agg(*prog.aggs)


def _row_tokens(rows, prog):
    out = {}
    for row in rows:
        assert row["k"] not in out
        out[row["k"]] = tuple(m.cell_token(struct.pack("<f", row[name]) if kind == m.hs.F32
                                           else row[name].to_bytes(4, "little", signed=True), kind)
                              for name, kind in zip(prog.names, prog.kinds))
    return out


_ORACLE_ROWS: dict = {}


@pytest.fixture(scope="module")
def engines():
    from minispark_amd.execution import HipExecutionEngine

    with HipExecutionEngine(0) as on, HipExecutionEngine(0) as off:
        off.short_tail_enabled = False
        yield {"short tail": on, "general tail": off}


@pytest.mark.parametrize("tail", ["short tail", "general tail"])
def test_whole_queries_over_the_quiet_scenarios_equal_the_oracle(engines, tmp_path, tail):
    """Four groups at a time: the private tables with the slab hand-over (hs_agg_partial_slab + the finish launch), or
    the general tail."""
    from minispark_amd.io import BlockFile
    from oracle.py_engine import run_query

    prog, engine = m.programs()["six"], engines[tail]
    finished_short = engine.short_tails
    for n, (scenarios, filler, live) in enumerate(m.LAUNCHES["narrow"][:5]):
        path = tmp_path / f"t{n}.bin"
        BlockFile(path).write_raw_blocks(m.SCHEMA, m.build_table(scenarios, filler, live, copies=False).blocks())
        if scenarios not in _ORACLE_ROWS:  # computed once, shared by both tails
            _ORACLE_ROWS[scenarios] = _row_tokens(run_query(_frame(object(), path, prog).task), prog)
        want = _ORACLE_ROWS[scenarios]
        assert _row_tokens(_frame(engine, path, prog).collect(), prog) == want, scenarios
        assert engine.dev.last_scan["tier"] == "private"
    assert engine.short_tails - finished_short == (5 if tail == "short tail" else 0), "the tail asked for is not the one that ran"


@pytest.mark.parametrize("tail", ["short tail", "general tail"])
def test_whole_queries_raise_what_the_oracle_raises(engines, tmp_path, tail):
    from minispark_amd.io import BlockFile

    for n, sc in enumerate(m.RAISING):
        for program, _flag, exception, _aggs in sc.raising[:1]:
            path = tmp_path / f"r{n}.bin"
            BlockFile(path).write_raw_blocks(m.SCHEMA, m.build_table((sc.name,), m.FILLER_KEYS[:1], True, copies=False).blocks())
            with pytest.raises(exception):
                _frame(engines[tail], path, m.programs()[program]).collect()
