"""The compiled private-tier scan resolves a quad's four group slots up front, folds the rows as straight-line code, runs
interior steps without liveness tests and compares a frame-of-reference date with a literal on the 16-bit delta
(DESIGN.md 4.1 / 4.5a).  None of that may change a bit of any result: every lane still folds its own rows into its own
cells in row order.

Each case runs a Q1-shaped query over a small table built for it and compares, bit for bit,
  * the compiled kernel over narrow columns (the path changed) with
  * the interpreter (HIPSPARK_JIT=0) and the stored columns (HIPSPARK_NARROW=0),
  * group keys and COUNT(*) with numpy, and
  * for the cases of ``_golden_cases`` with tests/golden/scan_rowstep.json: the result bits of the commit BEFORE the
    change, for the same seeded inputs (sums of 1e16, 1, -1e16 depend on the order of the folds).

The fixture was recorded once on an MI355X with the library of that commit:
    python -m tests.test_gpu_scan_rowstep tests/golden/scan_rowstep.json
"""

from __future__ import annotations

import ctypes as C
import json
import operator
import os
import sys
from contextlib import contextmanager
from datetime import datetime, timedelta
from pathlib import Path

import numpy as np
import pytest

from minispark_amd import hipspark as hs

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "scan_rowstep.json"
STEP = 1024  # rows of one workgroup step: 256 lanes x 4 rows
DAY_US = 86_400_000_000
BASE = 694_310_400_000_000  # 1992-01-02
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
QTY_POOL = np.array([1e16, 1.0, -1e16, 0.5, 3.0, 7.25], dtype=np.float32)  # few values: a LUT column; the sum depends on order
DISC_POOL = (np.arange(11, dtype=np.float32) / np.float32(100.0))
TAX_POOL = (np.arange(9, dtype=np.float32) / np.float32(100.0))


# ======================================================================================================================
# literals of any int64 value: the DataFrame API takes datetimes for a TIMESTAMP column; a placeholder datetime per value,
# mapped back where the lowering turns the literal into its 64-bit word
# ======================================================================================================================
_RAW: dict[datetime, int] = {}


def _lit(value: int):
    from minispark_amd.sql import Lit

    for dt, v in _RAW.items():
        if v == value:
            return Lit(dt)
    dt = datetime(2000, 1, 1) + timedelta(microseconds=len(_RAW))
    _RAW[dt] = int(value)
    return Lit(dt)


@contextmanager
def _raw_literals():
    from minispark_amd import lowering

    real = lowering.datetime_to_timestamp
    lowering.datetime_to_timestamp = lambda dt: _RAW[dt] if dt in _RAW else real(dt)
    try:
        yield
    finally:
        lowering.datetime_to_timestamp = real


@contextmanager
def _chunk_steps(steps: int | None):
    old = os.environ.get("HIPSPARK_CHUNK_STEPS")
    if steps is not None:
        os.environ["HIPSPARK_CHUNK_STEPS"] = str(steps)
    try:
        yield
    finally:
        if steps is not None:
            if old is None:
                del os.environ["HIPSPARK_CHUNK_STEPS"]
            else:
                os.environ["HIPSPARK_CHUNK_STEPS"] = old


# ======================================================================================================================
# tables and queries
# ======================================================================================================================
def _columns(n: int, seed: int, keys: np.ndarray | None = None, ship: np.ndarray | None = None,
             qty: np.ndarray | None = None) -> dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    return {
        "qty": QTY_POOL[rng.integers(0, len(QTY_POOL), n)] if qty is None else np.asarray(qty, np.float32),
        "price": (rng.integers(90_000, 10_000_000, n).astype(np.float32) / np.float32(100.0)),
        "disc": DISC_POOL[rng.integers(0, len(DISC_POOL), n)],
        "tax": TAX_POOL[rng.integers(0, len(TAX_POOL), n)],
        "flag": (np.frombuffer(b"ANR", np.uint8)[rng.integers(0, 3, n)] if keys is None else np.asarray(keys, np.uint8)),
        "ship": (BASE + DAY_US * rng.integers(0, 2526, n)).astype(np.int64) if ship is None else np.asarray(ship, np.int64),
    }


def _make_table(engine, root: Path, name: str, block_rows: list[int], cols: dict[str, np.ndarray]):
    import torch

    from minispark_amd import synth
    from minispark_amd.device import DCol
    from minispark_amd.io import BlockFile
    from minispark_amd.table import DeviceTable

    dev, n = engine.dev, sum(block_rows)
    assert all(len(v) == n for v in cols.values())
    path = root / f"{name}.bin"
    BlockFile(path, list(synth.LINEITEM_SCHEMA)).write_rows([])  # header only
    table = DeviceTable(path, list(synth.LINEITEM_SCHEMA), list(block_rows), {}, ())
    table.global_blocks, table.total_blocks = list(range(len(block_rows))), len(block_rows)
    for cid, key in ((1, "qty"), (2, "price"), (3, "disc"), (4, "tax")):
        table.columns[cid] = DCol(hs.F32, dev.to_device(cols[key], torch.float32), n)
    table.columns[5] = DCol(hs.STR, dev.to_device(cols["flag"], torch.uint8), n,
                            lens=dev.to_device(np.ones(n, np.uint8), torch.uint8), offs=None, fixed_len=1)
    table.columns[6] = DCol(hs.I64, dev.to_device(cols["ship"], torch.int64), n)
    engine.attach_device_table(path, table)
    return str(path), table


def _frame(engine, path: str, cond):
    from minispark_amd.workloads import engine_api

    api = engine_api(engine)
    Col, F, Lit = api.Col, api.F, api.Lit
    disc_price = Col("l_extendedprice") * (Lit(1) - Col("l_discount"))
    return (api.DataFrame().table(path).filter(cond).group_by(Col("l_returnflag"))
            .agg(F.sum(Col("l_quantity")).alias("q"), F.sum(Col("l_extendedprice")).alias("p"),
                 F.sum(disc_price * (Lit(1) + Col("l_tax"))).alias("c"), F.count().alias("n")))


def _ship():
    from minispark_amd.sql import Col

    return Col("l_shipdate")


def _canon(rows: list[dict]) -> list[dict]:
    """Rows ordered by key, floats as their exact hexadecimal text: equality is equality of bits."""
    return [{k: (v.hex() if isinstance(v, float) else v) for k, v in sorted(r.items())}
            for r in sorted(rows, key=lambda r: r["l_returnflag"])]


def _jit_launches(lib) -> int:
    counters = (C.c_int32 * 3)()
    lib.hs_jit_stats(counters)
    assert counters[2] == 0, lib.hs_jit_last_log()  # a program that does not compile would quietly run interpreted
    return counters[1]


@contextmanager
def _mode(engine, jit: bool, narrow: bool):
    lib = engine.dev._raw_lib
    engine.narrow_enabled = narrow
    if not jit:
        lib.hs_jit_set_enabled(0)
        engine.replay_enabled = False
    engine.dev._partial_prepared.clear()
    try:
        yield
    finally:
        lib.hs_jit_set_enabled(1)
        engine.replay_enabled = True
        engine.narrow_enabled = True
        engine.dev._partial_prepared.clear()


def _compiled(engine, frames: list, private: bool = True) -> list[list[dict]]:
    """The frames through the compiled kernel over narrow columns - and proof that it was that kernel."""
    lib = engine.dev._raw_lib
    out = []
    with _mode(engine, jit=True, narrow=True):
        for frame in frames:
            before = _jit_launches(lib)
            out.append(_canon(frame.collect()))
            launched = _jit_launches(lib) - before
            scan = engine.dev.last_scan
            if private:
                assert launched > 0, "the compiled kernel must have run"
                assert scan["tier"] == "private" and scan["wg_threads"] == 256 and scan["narrow_slots"], scan
    return out


def _other_modes(engine, frames: list, want: list[list[dict]]) -> None:
    lib = engine.dev._raw_lib
    with _mode(engine, jit=False, narrow=True):
        before = _jit_launches(lib)
        got = [_canon(f.collect()) for f in frames]
        assert _jit_launches(lib) == before, "the interpreter must have run"
    assert got == want, "compiled kernel against the interpreter"
    with _mode(engine, jit=True, narrow=False):
        got = [_canon(f.collect()) for f in frames]
        assert not engine.dev.last_scan["narrow_slots"]
    assert got == want, "narrow columns against the stored columns"


def _counts(cols: dict[str, np.ndarray], live: np.ndarray) -> dict[str, int]:
    keys, n = np.unique(cols["flag"][live], return_counts=True)
    return {bytes([int(k)]).decode(): int(c) for k, c in zip(keys, n)}


def _assert_counts(rows: list[dict], cols: dict[str, np.ndarray], live: np.ndarray) -> None:
    assert {r["l_returnflag"]: r["n"] for r in rows} == _counts(cols, live)


# ======================================================================================================================
# the cases whose bits the fixture pins
# ======================================================================================================================
CUTOFF = BASE + DAY_US * 1800
BLOCKS = [5, 1022, 1025, 3, 2050, 4097, 1, 3077, 6, 2047]  # unit boundaries that are no multiples of four


def _step_kinds(block_rows: list[int], steps_per_chunk: int) -> list[list[bool]]:
    """Per chunk, per step: is the step interior (all 1024 rows inside [unit begin, chunk end))?  Mirrors
    hs_agg_partial_chunks for 256 lanes."""
    out, start = [], 0
    for rows in block_rows:
        us, ue = start, start + rows
        start = ue
        for c0 in range(us & ~3, ue, STEP * steps_per_chunk):
            c1 = min(c0 + STEP * steps_per_chunk, ue)
            out.append([us <= s and s + STEP <= c1 for s in range(c0, c1, STEP)])
    return out


def _quad_keys(n: int) -> np.ndarray:
    """Quads AAAA, ABAB, ABCD in turn; the first quad of all is ABCD: four new keys at once."""
    pats = [b"ABCD", b"AAAA", b"ABAB"]
    return np.frombuffer(b"".join(pats[(i // 4) % 3] for i in range(0, n + 4, 4)), np.uint8)[:n].copy()


def _order_qty(n: int) -> np.ndarray:
    """1e16, 1, -1e16 mixes whose f64 sum depends on the order: a period of seven rows against the quads' four."""
    return np.array([1e16, 1.0, -1e16, 1.0, 1.0, -1e16, 1e16], dtype=np.float32)[np.arange(n) % 7]


def _where_patterns(n: int) -> tuple[np.ndarray, np.ndarray]:
    """Quad i keeps the rows named by the bits of i % 16 (none .. all four); every dropped row of quad 5 carries the key
    byte 'Q', which no kept row has: it must not reach the dictionary."""
    i = np.arange(n)
    keep = ((i // 4 % 16) >> (i % 4)) & 1 == 1
    ship = np.where(keep, CUTOFF - DAY_US * (i % 50), CUTOFF + DAY_US * (1 + i % 50)).astype(np.int64)
    keys = np.frombuffer(b"ANR", np.uint8)[i % 3].copy()
    keys[(i // 4 == 5) & ~keep] = ord("Q")
    return keys, ship


def _golden_cases() -> dict[str, dict]:
    cases: dict[str, dict] = {}
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4097):
        cases[f"rows_{n}"] = {"blocks": [n], "cols": _columns(n, 100 + n)}
    nb = sum(BLOCKS)
    for steps in (None, 3):
        cases[f"blocks_steps_{steps}"] = {"blocks": BLOCKS, "cols": _columns(nb, 7, qty=_order_qty(nb)), "steps": steps}
    n = 2 * STEP + 9
    cases["quad_key_patterns"] = {"blocks": [n], "cols": _columns(n, 8, keys=_quad_keys(n), qty=_order_qty(n))}
    late = np.full(STEP, ord("A"), np.uint8)
    late[STEP - 1] = ord("B")  # first seen in row 3 of the last lane's quad
    cases["key_first_seen_by_the_last_lane"] = {"blocks": [STEP], "cols": _columns(STEP, 9, keys=late, qty=_order_qty(STEP))}
    for distinct in (5, 17):  # the 4-slot table overflows: the run repeats, in the tier with room for the keys
        keys = (ord("a") + np.arange(3000) * 7 % distinct).astype(np.uint8)
        cases[f"distinct_keys_{distinct}"] = {"blocks": [1501, 1499], "cols": _columns(3000, distinct, keys=keys, qty=_order_qty(3000)),
                                              "private": False}
    n = 3 * STEP + 2
    keys, ship = _where_patterns(n)
    cases["where_patterns_in_a_quad"] = {"blocks": [n], "cols": _columns(n, 10, keys=keys, ship=ship, qty=_order_qty(n))}
    none = _columns(2050, 11)
    cases["no_row_kept"] = {"blocks": [2050], "cols": dict(none, ship=none["ship"] + DAY_US * 3000)}
    for n in (2047, 2045):  # the last step looks full: the rows behind the last one hold a key byte of their own
        cases[f"padding_{n}"] = {"blocks": [n], "cols": _columns(n, 12 + n, qty=_order_qty(n)), "poke": True}
    return cases


def _poke_padding(t, n: int, byte: int) -> None:
    """Fill what the buffer holds behind row n (the slack every device buffer carries) with `byte`."""
    import torch

    raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    raw[(t.storage_offset() + n) * t.element_size():] = byte


def _run_golden_case(engine, root: Path, name: str, case: dict, check_modes: bool) -> list[dict]:
    cols, n = case["cols"], sum(case["blocks"])
    with _raw_literals(), _chunk_steps(case.get("steps")):
        path, table = _make_table(engine, root, name, case["blocks"], cols)
        frame = _frame(engine, path, _ship() <= _lit(CUTOFF))
        if case.get("poke"):
            frame.collect()  # (the narrow forms exist from here on)
            _poke_padding(table.columns[5].data, n, ord("Z"))
            _poke_padding(table.columns[2].data, n, 0x41)  # a price of 12.08
            for cid in (1, 3, 4, 6):
                _poke_padding(table.columns[cid].data, n, 0)  # 1970-01-01: it would pass the WHERE
                if table.columns[cid].narrow is not None:
                    _poke_padding(table.columns[cid].narrow.data, n, 0xFF if cid != 6 else 0)
        (got,) = _compiled(engine, [frame], private=case.get("private", True))
        if case.get("steps") is not None:
            assert engine.dev.last_scan["chunk_rows"] == STEP * case["steps"]
        if check_modes:
            _other_modes(engine, [frame], [got])
    _assert_counts(got, cols, cols["ship"] <= CUTOFF)
    return got


@pytest.fixture(scope="module")
def engine(tmp_path_factory):
    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine

    constants.SHUFFLE_FOLDER = tmp_path_factory.mktemp("rowstep") / "shuffle"
    eng = HipExecutionEngine(0)
    assert eng.narrow_enabled
    yield eng
    eng.__exit__(None, None, None)


@pytest.fixture(scope="module")
def golden() -> dict:
    return json.loads(GOLDEN.read_text())


def test_the_block_table_holds_the_chunk_shapes_it_is_there_for():
    starts = np.cumsum([0] + BLOCKS[:-1])
    assert sum(1 for s in starts if s % 4) >= 6
    one = _step_kinds(BLOCKS, 1)  # what a small table gets: one step per chunk
    assert [False] in one and [True] in one
    three = _step_kinds(BLOCKS, 3)
    assert any(len(k) >= 2 and not any(k) for k in three), "a chunk of edge steps only"
    assert [False, True, False] in three, "a chunk with exactly one interior step"


@pytest.mark.parametrize("name", list(_golden_cases()))
def test_result_bits_are_those_of_the_row_at_a_time_scan(engine, golden, tmp_path, name):
    got = _run_golden_case(engine, tmp_path, name, _golden_cases()[name], check_modes=True)
    assert got == golden[name]
    if name == "where_patterns_in_a_quad":
        assert "Q" not in {r["l_returnflag"] for r in got}
    if name.startswith("padding"):
        assert "Z" not in {r["l_returnflag"] for r in got}
    if name == "no_row_kept":
        assert got == []


# ======================================================================================================================
# WHERE on the frame-of-reference column in the code domain
# ======================================================================================================================
def _for_tables() -> dict[str, tuple[int, int, int]]:
    """name -> (base, scale, largest delta)"""
    return {"days": (BASE, DAY_US, 2525), "negative_base": (-10**15, 7, 65_535), "range_65535": (-5, 1, 65_535)}


def _for_literals(base: int, scale: int, top: int) -> list[int]:
    mx = base + scale * top
    return [base - 1, base, base + scale - 1, base + scale, mx, mx + 1, I64_MIN, I64_MAX, base + scale * (top // 2) + scale // 2]


def _for_columns(base: int, scale: int, top: int, n: int, seed: int) -> dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    k = rng.integers(0, top + 1, n)
    k[:3] = [0, top, 1]  # both ends, and two neighbours: the encoder finds this base and this scale
    ship = np.array([base + scale * int(x) for x in rng.permutation(k)], dtype=np.int64)
    return _columns(n, seed, ship=ship)


FORMS = [(op, mirrored) for mirrored in (False, True) for op in ("le", "lt", "ge", "gt")]


@pytest.mark.parametrize("op,mirrored", FORMS, ids=[f"{'lit_' if m else 'col_'}{o}" for o, m in FORMS])
def test_for_compare_on_the_delta(engine, tmp_path, op, mirrored):
    fn = getattr(operator, op)
    with _raw_literals():
        for tname, (base, scale, top) in _for_tables().items():
            cols = _for_columns(base, scale, top, 1500, 33)
            path, table = _make_table(engine, tmp_path, f"{tname}_{op}_{int(mirrored)}", [701, 799], cols)
            lits = _for_literals(base, scale, top)
            frames = [_frame(engine, path, fn(_lit(v), _ship()) if mirrored else fn(_ship(), _lit(v))) for v in lits]
            got = _compiled(engine, frames)
            assert table.columns[6].narrow is not None and table.columns[6].narrow.kind == hs.I64_FOR16
            params = table.columns[6].narrow.offs.cpu().numpy()
            assert (int(params[0]), int(params[1])) == (base, scale)
            for v, rows in zip(lits, got):
                live = fn(np.int64(v), cols["ship"]) if mirrored else fn(cols["ship"], np.int64(v))
                _assert_counts(rows, cols, live)
            _other_modes(engine, frames, got)


def test_for_compare_in_the_keyless_kernel(engine, tmp_path):
    from minispark_amd.workloads import engine_api

    api = engine_api(engine)
    Col, F = api.Col, api.F
    base, scale, top = _for_tables()["negative_base"]
    cols = _for_columns(base, scale, top, 2500, 34)
    with _raw_literals():
        path, _table = _make_table(engine, tmp_path, "keyless", [1203, 1297], cols)
        lo, hi = base + scale * 20_000 + 3, base + scale * 40_000
        frames = [api.DataFrame().table(path).filter((Col("l_shipdate") >= _lit(a)) & (_lit(b) > Col("l_shipdate")))
                  .agg(F.sum(Col("l_extendedprice") * Col("l_discount")).alias("r"), F.count().alias("n"))
                  for a, b in ((lo, hi), (I64_MIN, hi), (lo, I64_MAX), (hi, lo))]
        lib = engine.dev._raw_lib
        got = []
        with _mode(engine, jit=True, narrow=True):
            for f in frames:
                before = _jit_launches(lib)
                got.append(f.collect())
                assert _jit_launches(lib) > before and engine.dev.last_scan["tier"] == "scalar"
                assert engine.dev.last_scan["narrow_slots"]
        for (a, b), rows in zip(((lo, hi), (I64_MIN, hi), (lo, I64_MAX), (hi, lo)), got):
            n = int(((cols["ship"] >= a) & (cols["ship"] < b)).sum())
            assert (rows[0]["n"] if rows else 0) == n
        with _mode(engine, jit=False, narrow=True):
            assert [f.collect() for f in frames] == got
        with _mode(engine, jit=True, narrow=False):
            assert [f.collect() for f in frames] == got


# ======================================================================================================================
# recording the fixture (see the module docstring)
# ======================================================================================================================
def _record(out: Path) -> None:
    import tempfile

    from minispark_amd import constants
    from minispark_amd.execution import HipExecutionEngine

    root = Path(tempfile.mkdtemp(prefix="rowstep_"))
    constants.SHUFFLE_FOLDER = root / "shuffle"
    with HipExecutionEngine(0) as eng:
        rows = {name: _run_golden_case(eng, root, name, case, check_modes=False) for name, case in _golden_cases().items()}
    out.write_text(json.dumps(rows, indent=1, sort_keys=True) + "\n")
    print(f"{len(rows)} cases -> {out}")


if __name__ == "__main__":
    _record(Path(sys.argv[1]))
