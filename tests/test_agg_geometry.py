"""Host layer of the aggregate scans (csrc/hs_agg.hip) without a GPU: the three *_geom entries, the chunk table and the
launchers' refusals answer what tests/golden/agg_geometry.json recorded before that layer was reorganised; the
computed-units geometry follows the rule include/hipspark.h states for it."""

from __future__ import annotations

import ctypes as C
import importlib.util
import json

import pytest

from minispark_amd import hipspark as hs
from tests.conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_agg_geometry", ROOT / "tests" / "golden" / "make_agg_geometry.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded() -> dict:
    return json.loads((ROOT / "tests" / "golden" / "agg_geometry.json").read_text())


def _inputs(case: dict) -> dict:
    return {k: v for k, v in case.items() if k != "want"}


def test_every_geometry_and_chunk_table_equals_the_recording(recorded):
    lib = hs.load_library()
    assert [_inputs(c) for c in recorded["geometry"]] == gen.geometry_cases()  # the recording covers today's case list
    outcomes = {c["want"]["rc"] for c in recorded["geometry"]}
    assert outcomes == {0, 1, 2}  # fits / bad arguments (n_acc 0 keyless, group_cap 3) / HS_E_LIMIT
    for case in recorded["geometry"]:
        assert gen.run_geometry(lib, _inputs(case)) == case["want"], _inputs(case)


def test_every_refusal_equals_the_recording(recorded):
    lib = hs.load_library()
    assert [_inputs(c) for c in recorded["refusals"]] == gen.refusal_cases()
    for case in recorded["refusals"]:
        assert case["want"]["rc"] in (1, 2) and case["want"]["error"]
        assert gen.run_refusal(lib, _inputs(case)) == case["want"], _inputs(case)


def test_computed_units_geometry_follows_the_rule_in_the_header(recorded):
    """hs_agg_shared_units_geom = the recorded hs_agg_shared_geom over [0, nrows) with pad lowered to the per-unit share
    and ws_bytes in the two forms the launchers index (hipspark.h); nothing here is taken from the entry itself."""
    lib = hs.load_library()
    shared = {(c["units"], c["n_acc"], c["group_cap"]): c["want"] for c in recorded["geometry"]
              if c["entry"] == "hs_agg_shared_geom"}
    ranges = [name for name, bounds in gen.UNIT_LISTS.items() if len(bounds) == 2]
    assert len(ranges) == 4
    geom = hs.hs_agg_geom()
    seen = set()
    for name in ranges:
        nrows = gen.UNIT_LISTS[name][1]
        for n_acc in gen.N_ACCS:
            for cap in gen.GROUP_CAPS:
                base = shared[(name, n_acc, cap)]
                for tables in (1, 10, 127):
                    for caller_keys in (0, 1):
                        rc = lib.hs_agg_shared_units_geom(nrows, tables, n_acc, cap, caller_keys, C.byref(geom))
                        assert rc == base["rc"], (name, n_acc, cap, tables)
                        seen.add(rc)
                        if rc:
                            continue
                        group_cap, chunk_rows, wg, pad, n_chunks, lds, _ = base["geom"]
                        share = 16
                        while share < 4 * max(4, cap // tables):
                            share *= 2
                        pad = min(pad, share)
                        keys = 0 if caller_keys else (tables * pad * 8 + 256 + 15) // 16 * 16
                        ws = keys + max(n_chunks, 1) * tables * pad * max(n_acc, 1) * 8
                        got = [int(getattr(geom, f)) for f, _ in hs.hs_agg_geom._fields_]
                        assert got == [group_cap, chunk_rows, wg, pad, n_chunks, lds, ws], (name, n_acc, cap, tables, caller_keys)
    assert seen == {0, 1, 2}
    for nrows, tables, out in ((100, 0, C.byref(geom)), (100, 128, C.byref(geom)), (-1, 3, C.byref(geom)), (100, 3, None)):
        assert lib.hs_agg_shared_units_geom(nrows, tables, 2, 16, 0, out) == 1
        assert b"hs_agg_shared_units_geom" in lib.hs_last_error()
