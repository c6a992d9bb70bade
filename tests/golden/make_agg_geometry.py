"""Golden for the aggregate scans' host layer (csrc/hs_agg.hip): what the three *_geom entries, hs_agg_partial_chunks and
the launchers' argument checks answer.  Pure host arithmetic - no GPU, no reference code:

    python tests/golden/make_agg_geometry.py

writes tests/golden/agg_geometry.json from the library as built.  Recorded ONCE, before the host layer was reorganised;
tests/test_agg_geometry.py runs the same cases (it imports them from here) and compares.  Re-record only when a
geometry rule or a refusal is changed on purpose."""

from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from minispark_amd import hipspark as hs  # noqa: E402

OUT = HERE / "agg_geometry.json"

# ---- geometry ----------------------------------------------------------------------------------------------------------
UNIT_LISTS = {
    "empty": [0, 0],
    "one_row": [0, 1],
    "ragged": [0, 5, 5, 4103, 70001],  # an empty unit, starts off a multiple of 4
    "3x2000405": [i * 2_000_405 for i in range(4)],
    "287x2090724": [i * 2_090_724 for i in range(288)],
    "two_chunks": [0, 65536 + 4100],
    "60M": [0, 60_000_000],
}
N_ACCS = (0, 1, 6, 16)
GROUP_CAPS = (1, 3, 4, 64, 1024, 8192)  # 3: not a power of two; the large ones reach HS_E_LIMIT


def geometry_cases() -> list[dict]:
    cases = []
    for name in UNIT_LISTS:
        for n_acc in N_ACCS:
            cases.append({"entry": "hs_agg_scalar_geom", "units": name, "n_acc": n_acc, "group_cap": 1, "chunk_steps": None})
            for entry in ("hs_agg_partial_geom", "hs_agg_shared_geom"):
                for cap in GROUP_CAPS:
                    cases.append({"entry": entry, "units": name, "n_acc": n_acc, "group_cap": cap, "chunk_steps": None})
    cases.append({"entry": "hs_agg_partial_geom", "units": "3x2000405", "n_acc": 6, "group_cap": 4, "chunk_steps": 7})
    return cases


def run_geometry(lib, case: dict) -> dict:
    """-> {"rc"} or {"rc": 0, "geom": [7 fields], "chunks": ...} for one case."""
    bounds = UNIT_LISTS[case["units"]]
    n_units = len(bounds) - 1
    units = (C.c_int64 * len(bounds))(*bounds)
    geom = hs.hs_agg_geom()
    os.environ.pop("HIPSPARK_CHUNK_STEPS", None)
    if case["chunk_steps"] is not None:
        os.environ["HIPSPARK_CHUNK_STEPS"] = str(case["chunk_steps"])
    try:
        if case["entry"] == "hs_agg_scalar_geom":
            rc = lib.hs_agg_scalar_geom(units, n_units, case["n_acc"], C.byref(geom))
        else:
            rc = getattr(lib, case["entry"])(units, n_units, case["n_acc"], case["group_cap"], C.byref(geom))
    finally:
        os.environ.pop("HIPSPARK_CHUNK_STEPS", None)
    if rc != 0:
        return {"rc": rc}
    fields = [int(getattr(geom, f)) for f, _ in hs.hs_agg_geom._fields_]
    return {"rc": 0, "geom": fields, "chunks": chunk_table(lib, units, n_units, geom)}


def chunk_table(lib, units, n_units: int, geom) -> dict:
    chunks = np.zeros((max(int(geom.n_chunks), 1), 4), dtype=np.int64)
    chunk0 = np.zeros(n_units + 1, dtype=np.int64)
    rc = lib.hs_agg_partial_chunks(units, n_units, C.byref(geom), chunks.ctypes.data_as(C.POINTER(hs.hs_chunk)),
                                   chunk0.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        return {"rc": rc}
    chunks = chunks[: int(geom.n_chunks)]
    if len(chunks) <= 16:
        return {"rc": 0, "rows": chunks.tolist(), "unit_chunk0": chunk0.tolist()}
    digest = hashlib.sha256(chunks.tobytes() + chunk0.tobytes()).hexdigest()
    return {"rc": 0, "n_chunks": len(chunks), "first": chunks[0].tolist(), "last": chunks[-1].tolist(), "sha256": digest}


# ---- refusals: host structs, dummy non-null device pointers, every case fails before any launch ---------------------------
LAUNCHERS = ("hs_agg_partial", "hs_agg_partial_slab", "hs_agg_scalar", "hs_agg_shared", "hs_agg_shared_units",
             "hs_agg_shared_join8")
KEYED = ("hs_agg_partial", "hs_agg_partial_slab", "hs_agg_shared", "hs_agg_shared_units", "hs_agg_shared_join8")
FAULTS = {
    "program_too_long": LAUNCHERS,
    "ninth_numeric_slot": LAUNCHERS,
    # (HS_JOIN8_* in the private-table tier is not refused: the call reaches a launch, so it is not a case here)
    "pair_column": ("hs_agg_partial", "hs_agg_partial_slab", "hs_agg_scalar"),
    "pair_column_without_rows": ("hs_agg_shared", "hs_agg_shared_units", "hs_agg_shared_join8"),
    "join8_column": ("hs_agg_scalar", "hs_agg_shared", "hs_agg_shared_units"),
    "narrow_key": KEYED,
    "narrow_column_without_parameters": ("hs_agg_partial", "hs_agg_scalar", "hs_agg_shared", "hs_agg_shared_units",
                                         "hs_agg_shared_join8"),
    "narrow_column_read_by_strcmp": ("hs_agg_partial", "hs_agg_scalar"),
    "stack_too_deep": LAUNCHERS,
    "foreign_geometry": LAUNCHERS,
    "keyless_program_with_key": ("hs_agg_scalar",),
    "accumulator_never_fed": ("hs_agg_scalar",),
}


def refusal_cases() -> list[dict]:
    return [{"launcher": launcher, "fault": fault} for fault, launchers in FAULTS.items() for launcher in launchers]


def _ins(op: int, sp: int = 0, a: int = 0, b: int = 0) -> int:
    return op | (sp << 8) | (a << 16) | (b << 32)


def run_refusal(lib, case: dict) -> dict:
    launcher, fault = case["launcher"], case["fault"]
    keyless = launcher == "hs_agg_scalar"
    units_form = launcher in ("hs_agg_shared_units", "hs_agg_shared_join8")
    raw = (C.c_uint8 * 4096)()
    dummy = (C.addressof(raw) + 255) & ~255  # never read: every case returns before a launch
    # slots: [key] value [unit]; the keyless tier has no key column
    n_cols = (1 if keyless else 2) + (1 if units_form else 0)
    value, unit = (0 if keyless else 1), n_cols - 1
    cols = (hs.hs_col * hs.HS_MAX_COLS)()
    for i in range(hs.HS_MAX_COLS):
        cols[i].kind, cols[i].fixed_len, cols[i].data = hs.F32, -1, dummy
    if not keyless:
        cols[0].kind = hs.I32
    if units_form:
        cols[unit].kind = hs.U8 if launcher == "hs_agg_shared_units" else hs.JOIN8_UNIT
    prog = hs.hs_program()
    ins = [_ins(hs.OP_LD, 0, value), _ins(hs.OP_AGG, 0, 0)]
    spec = hs.hs_agg_spec()
    spec.n_acc = 1
    spec.op[0], spec.is_int[0] = hs.AGG_SUM, 0
    bounds = (C.c_int64 * 2)(0, 100_000)
    geom = hs.hs_agg_geom()
    own = {"hs_agg_scalar": "scalar", "hs_agg_partial": "partial", "hs_agg_partial_slab": "partial"}.get(launcher, "shared")
    made_by = own
    if fault == "foreign_geometry":
        made_by = "shared" if own == "partial" else "partial"
    if fault == "accumulator_never_fed":
        spec.n_acc = 2
        spec.op[1] = hs.AGG_MIN
    if made_by == "scalar":
        rc = lib.hs_agg_scalar_geom(bounds, 1, spec.n_acc, C.byref(geom))
    elif made_by == "partial":
        rc = lib.hs_agg_partial_geom(bounds, 1, spec.n_acc, 4, C.byref(geom))
    else:
        rc = lib.hs_agg_shared_geom(bounds, 1, spec.n_acc, 16, C.byref(geom))
    assert rc == 0 and geom.n_chunks > 0, lib.hs_last_error()

    if fault == "program_too_long":
        prog.n_ins = hs.HS_MAX_INS + 1
    elif fault == "ninth_numeric_slot":
        n_cols = hs.HS_FUSED_COLS + 2  # the unit column keeps its preloaded slot; slots 8, 9 are FLOAT columns
    elif fault in ("pair_column", "pair_column_without_rows"):
        cols[value].kind = hs.F32 | hs.PAIR  # (offs stays NULL: the shared tier wants the pair rows there)
    elif fault == "join8_column":
        cols[value].kind = hs.JOIN8_CODE
    elif fault == "narrow_key":
        cols[0].kind, cols[0].offs = hs.I64_FOR16, dummy
    elif fault == "narrow_column_without_parameters":
        cols[value].kind = hs.I64_FOR16
    elif fault == "narrow_column_read_by_strcmp":
        cols[value].kind, cols[value].offs = hs.I64_FOR16, dummy
        ins = [_ins(hs.OP_STRCMP_LIT, 0, value), _ins(hs.OP_FILTER, 0)] + ins
    elif fault == "stack_too_deep":
        ins = [_ins(hs.OP_LD, sp, value) for sp in range(hs.HS_MAX_STACK + 1)] + [_ins(hs.OP_AGG, 0, 0)]
    elif fault == "keyless_program_with_key":
        ins = [_ins(hs.OP_LD, 0, value), _ins(hs.OP_KEY, 0)] + ins
    if fault != "program_too_long":
        prog.n_ins = len(ins)
        for i, w in enumerate(ins):
            prog.ins[i] = w

    p, byref = dummy, C.byref
    if launcher == "hs_agg_partial":
        rc = lib.hs_agg_partial(None, cols, n_cols, 0, byref(prog), byref(spec), p, p, 1, byref(geom), p, p, p, p, p, None, None)
    elif launcher == "hs_agg_partial_slab":
        desc = hs.hs_slab_desc()
        desc.slab_rows, desc.key_kind, desc.key_len, desc.n_acc = 1 << 20, cols[0].kind, 0, spec.n_acc
        desc.acc_kind[0] = hs.F32
        rc = lib.hs_agg_partial_slab(None, cols, n_cols, 0, byref(prog), byref(spec), p, p, 1, byref(geom), None, p, byref(desc),
                                     p, p, None, None)
    elif launcher == "hs_agg_scalar":
        rc = lib.hs_agg_scalar(None, cols, n_cols, byref(prog), byref(spec), p, p, 1, byref(geom), p, p, p, p, p, p, None, None)
    elif launcher == "hs_agg_shared":
        rc = lib.hs_agg_shared(None, cols, n_cols, 0, byref(prog), byref(spec), p, 1, byref(geom), p, p, p, p, p, None, None)
    elif launcher == "hs_agg_shared_units":
        rc = lib.hs_agg_shared_units(None, cols, n_cols, 0, unit, 3, byref(prog), byref(spec), p, byref(geom), p, p, p, p, p,
                                     None, None)
    else:
        join = hs.hs_join8(dummy, 1, 0, 3)
        rc = lib.hs_agg_shared_join8(None, cols, n_cols, 0, unit, byref(join), 3, byref(prog), byref(spec), p, byref(geom), p,
                                     p, p, p, p, None, None)
    return {"rc": rc, "error": lib.hs_last_error().decode() if rc else ""}


def main() -> None:
    lib = hs.load_library()
    geometry = [{**case, "want": run_geometry(lib, case)} for case in geometry_cases()]
    refusals = [{**case, "want": run_refusal(lib, case)} for case in refusal_cases()]
    bad = [r for r in refusals if r["want"]["rc"] == 0]
    assert not bad, f"not refused: {bad}"
    lines = ["{", '"geometry": [']
    lines += [json.dumps(c) + ("," if i + 1 < len(geometry) else "") for i, c in enumerate(geometry)]
    lines += ["],", '"refusals": [']
    lines += [json.dumps(c) + ("," if i + 1 < len(refusals) else "") for i, c in enumerate(refusals)]
    lines += ["]", "}"]
    OUT.write_text("\n".join(lines) + "\n")
    print(OUT.name, len(geometry), "geometry cases,", len(refusals), "refusals,", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
