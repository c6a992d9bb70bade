"""Narrow column kinds (HS_I64_FOR16 / HS_F32_LUT8) on the GPU: the encoder round trip through the C ABI,
and the fused scan over narrow columns against the same scan over the stored columns - bit for bit, through the compiled
kernel, the interpreter and a replayed recording - and against the C oracle."""

from __future__ import annotations

import ctypes as C
import math
from datetime import datetime

import numpy as np
import pytest
import torch

from minispark_amd import hipspark as hs
from tests.conftest import assert_rows_match

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
ROWS, PER_BLOCK, SEED = 300_000, 65_533, 20251003  # unit starts are not multiples of 4
CUTOFFS = ["1998-12-01", "1998-09-02", "1994-03-15", "1991-01-01"]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def dev():
    from minispark_amd.device import Device

    return Device(0)


# ======================================================================================================================
# encoder round trip (C ABI)
# ======================================================================================================================
def _lut8(dev, bits: np.ndarray):
    """hs_narrow_lut8 over the f32 column with these bit patterns -> (entries, table bits, codes)."""
    n = len(bits)
    data = dev.to_device(bits.view(np.float32), torch.float32)
    codes = dev.empty(n, torch.uint8)
    lut = torch.zeros(256, dtype=torch.float32, device=dev.device)
    ws = dev.workspace(dev.lib.hs_narrow_ws_bytes())
    entries = C.c_int32(-1)
    hs.check(dev.lib.hs_narrow_lut8(dev.stream, data.data_ptr(), n, codes.data_ptr(), lut.data_ptr(), ws.data_ptr(),
                                    C.byref(entries)), "hs_narrow_lut8")
    return entries.value, lut.cpu().numpy().view(np.uint32), codes.cpu().numpy()


def _pattern_pool(k: int) -> np.ndarray:
    """k distinct f32 bit patterns: +0.0 and -0.0 first, then two NaN payloads, the infinities, a denormal, FLT_MAX, then
    ordinary values."""
    special = [0x00000000, 0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF]
    ordinary = (np.arange(1, 400, dtype=np.float32) / np.float32(100.0)).view(np.uint32).tolist()
    pool = np.array((special + ordinary)[:k], dtype=np.uint32)
    assert len(np.unique(pool)) == k
    return pool


@pytest.mark.parametrize("n", SIZES)
def test_lut8_round_trip_is_bit_exact(dev, n):
    rng = np.random.default_rng(n)
    for k in (1, 2, 255, 256):
        pool = _pattern_pool(k)
        bits = pool[rng.permutation(np.arange(n) % k)]  # every pattern the size allows, in no order
        want = np.unique(bits)
        entries, lut, codes = _lut8(dev, bits)
        assert entries == len(want), (n, k)
        assert lut[:entries].tobytes() == want.tobytes(), (n, k)  # keyed by bit pattern, ascending: independent of row order
        assert lut[codes].tobytes() == bits.tobytes(), (n, k)
    if n >= 257:
        bits = _pattern_pool(257)[rng.permutation(np.arange(n) % 257)]
        assert _lut8(dev, bits)[0] == 0, "a 257th pattern: not eligible"


def _for16_model(values: list[int]):
    """The eligibility rule in Python integers (no width, no wrap): (eligible, base, scale)."""
    g = 0
    for v in values:
        g = math.gcd(g, v - values[0])
    scale = g or 1
    mn, mx = min(values), max(values)
    return (mx - mn) <= I64_MAX and (mx - mn) // scale <= 65535, mn, scale


def _for16(dev, values: np.ndarray):
    n = len(values)
    data = dev.to_device(values, torch.int64)
    codes = dev.empty(n, torch.int16)
    params = torch.zeros(2, dtype=torch.int64, device=dev.device)
    ws = dev.workspace(dev.lib.hs_narrow_ws_bytes())
    ok = C.c_int32(-1)
    hs.check(dev.lib.hs_narrow_for16(dev.stream, data.data_ptr(), n, codes.data_ptr(), params.data_ptr(), ws.data_ptr(),
                                     C.byref(ok)), "hs_narrow_for16")
    return ok.value, params.cpu().numpy(), codes.cpu().numpy().view(np.uint16)


DAY_US = 86_400_000_000


def _for16_cases(n: int, rng) -> dict[str, tuple[np.ndarray, bool | None]]:
    """name -> (column, the answer the case stands for once the column is long enough to show it, else None)."""
    long_enough = n >= 3

    def spread(lo: int, step: int, top: int) -> np.ndarray:
        """lo + step * k with k = 0, 1 and `top` present (when n >= 3) and the rest random below top."""
        k = rng.integers(0, top + 1, n)
        k[: min(n, 3)] = [0, top, 1][: min(n, 3)]
        return np.array([lo + step * int(x) for x in rng.permutation(k)], dtype=np.int64)

    return {
        "day multiples": (spread(694_310_400_000_000, DAY_US, 2525), True),
        "gcd 1": (spread(1_000_000_007, 1, 40_000), True),
        "range 65535": (spread(-5, 1, 65_535), True),
        "range 65536": (spread(-5, 1, 65_536), False if long_enough else None),
        "negative base": (spread(-10**15, 7, 65_535), True),
        "one value": (np.full(n, -123_456_789_012, dtype=np.int64), True),
        "int64 extremes": (np.array(([I64_MIN, I64_MAX] * n)[:n], dtype=np.int64), False if n >= 2 else None),
    }


@pytest.mark.parametrize("n", SIZES)
def test_for16_round_trip_is_exact_and_ranges_are_refused_not_wrapped(dev, n):
    for name, (values, stands_for) in _for16_cases(n, np.random.default_rng(100 + n)).items():
        eligible, base, scale = _for16_model([int(v) for v in values])
        if stands_for is not None:
            assert eligible == stands_for, (name, n, "the case does not show what it is named for")
        ok, params, codes = _for16(dev, values)
        assert bool(ok) == eligible, (name, n)
        if not eligible:
            continue
        assert (int(params[0]), int(params[1])) == (base, scale), (name, n)
        decoded = [base + int(c) * scale for c in codes]
        assert decoded == [int(v) for v in values], (name, n)
        if name == "day multiples":
            assert scale % DAY_US == 0 or n == 1  # (a one-row column is one-valued: gcd 0, scale 1)
        if name == "one value":
            assert scale == 1 and not codes.any()
        if name == "negative base":
            assert base < 0 and (scale == 7 or n < 3)


def test_empty_columns_are_not_eligible(dev):
    ok = C.c_int32(-1)
    hs.check(dev.lib.hs_narrow_for16(dev.stream, None, 0, None, None, None, C.byref(ok)), "hs_narrow_for16")
    assert ok.value == 0
    hs.check(dev.lib.hs_narrow_lut8(dev.stream, None, 0, None, None, None, C.byref(ok)), "hs_narrow_lut8")
    assert ok.value == 0


# ======================================================================================================================
# the scan over narrow columns (engine)
# ======================================================================================================================
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from minispark_amd import constants, synth
    from minispark_amd.execution import HipExecutionEngine
    from oracle import q1_native

    root = tmp_path_factory.mktemp("narrow")
    constants.SHUFFLE_FOLDER = root / "shuffle"
    engine = HipExecutionEngine(0)
    assert engine.narrow_enabled
    path = root / "lineitem.bin"
    table = synth.make_lineitem(engine.dev, path, ROWS, rows_per_block=PER_BLOCK, with_orderkey=True)
    engine.attach_device_table(path, table)
    cols = q1_native.gen(SEED, 0, ROWS)  # the CPU twin of the generator, once for every test below
    yield engine, str(path), table, cols
    engine.__exit__(None, None, None)


def _api(engine):
    from minispark_amd.workloads import engine_api

    return engine_api(engine)


def _oracle(cols, block_rows, cutoff):
    from oracle import blockfile as bfio
    from oracle import q1_native

    return q1_native.run(cols, block_rows, bfio.to_us(datetime.fromisoformat(cutoff)), threads=4)


def _jit_launches(lib) -> int:
    counters = (C.c_int32 * 3)()
    lib.hs_jit_stats(counters)
    assert counters[2] == 0, lib.hs_jit_last_log()
    return counters[1]


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_q1_over_narrow_columns_is_bit_identical(setup, cutoff):
    from minispark_amd.workloads import q1

    engine, path, table, cols = setup
    lib = engine.dev._raw_lib
    want = _oracle(cols, table.block_rows, cutoff)

    engine.narrow_enabled = True
    frame = q1(_api(engine), path, cutoff)
    launches = _jit_launches(lib)
    narrow = frame.collect()
    assert _jit_launches(lib) > launches, "the compiled kernel must have run"
    scan = engine.dev.last_scan
    assert scan["moved_bytes_per_row"] == 10 and len(scan["narrow_slots"]) == 4 and scan["tier"] == "private"
    assert scan["group_cap"] == 4 and scan["wg_threads"] == 256
    for cid, kind in ((1, hs.F32_LUT8), (3, hs.F32_LUT8), (4, hs.F32_LUT8), (6, hs.I64_FOR16)):
        assert table.columns[cid].narrow.kind == kind and table.columns[cid].kind in (hs.F32, hs.I64)
    assert table.columns[2].narrow is None  # l_extendedprice: too many values
    assert [table.columns[c].narrow.fixed_len for c in (1, 3, 4)] == [50, 11, 9]
    assert table.stored_column(6).data.dtype == torch.int64  # what every other consumer sees is the stored column
    assert_rows_match(narrow, want, max_ulps=1)

    # a recorded run and its replay
    replays = engine.replays
    recorded = frame.collect()
    replayed = frame.collect()
    assert engine.replays > replays, "the third run replays the second's recording"
    assert engine.dev.last_scan["moved_bytes_per_row"] == 10
    assert narrow == recorded == replayed

    # the stored columns
    engine.narrow_enabled = False
    plain = q1(_api(engine), path, cutoff).collect()
    assert engine.dev.last_scan["moved_bytes_per_row"] == 25 and engine.dev.last_scan["narrow_slots"] == []
    assert narrow == plain, "narrow columns decode exactly: the same bits, not merely the same ulp"
    assert frame.collect() == plain and engine.dev.last_scan["moved_bytes_per_row"] == 25  # (the switch is part of every key)
    engine.narrow_enabled = True

    # the interpreter over the narrow columns
    lib.hs_jit_set_enabled(0)
    engine.replay_enabled = False
    try:
        engine.dev._partial_prepared.clear()
        launches = _jit_launches(lib)
        interp = frame.collect()
        assert _jit_launches(lib) == launches, "the interpreter kernel must have run"
        assert engine.dev.last_scan["moved_bytes_per_row"] == 10
    finally:
        lib.hs_jit_set_enabled(1)
        engine.replay_enabled = True
        engine.dev._partial_prepared.clear()
    assert narrow == interp
    if cutoff == "1991-01-01":
        assert narrow == []


def test_keyless_tier_over_narrow_columns(setup):
    from minispark_amd.workloads import q6

    engine, path, table, cols = setup
    engine.narrow_enabled = True
    frame = q6(_api(engine), path)
    narrow = frame.collect()
    scan = engine.dev.last_scan
    assert scan["tier"] == "scalar" and len(scan["narrow_slots"]) == 3 and scan["moved_bytes_per_row"] == 2 + 1 + 1 + 4
    assert frame.collect() == narrow and frame.collect() == narrow  # recorded, replayed
    engine.narrow_enabled = False
    try:
        plain = q6(_api(engine), path).collect()
        assert engine.dev.last_scan["moved_bytes_per_row"] == 20
    finally:
        engine.narrow_enabled = True
    assert narrow == plain and len(narrow) == 1 and narrow[0]["revenue"] > 0
    lib = engine.dev._raw_lib
    lib.hs_jit_set_enabled(0)
    engine.replay_enabled = False
    try:
        engine.dev._partial_prepared.clear()
        assert frame.collect() == narrow
    finally:
        lib.hs_jit_set_enabled(1)
        engine.replay_enabled = True
        engine.dev._partial_prepared.clear()


def test_other_tiers_and_hs_eval_see_the_stored_columns(setup):
    """A GROUP BY with tens of thousands of groups leaves the private-table tier: it reads plain columns whatever the
    switch says; so does an expression evaluated over the table."""
    from minispark_amd import table as tbl
    from minispark_amd.sql import Col, Functions as F

    engine, path, table, cols = setup
    api = _api(engine)

    def build():
        return (api.DataFrame().table(path).filter(Col("l_shipdate") <= "1998-09-02").group_by(Col("l_orderkey"))
                .agg(F.sum(Col("l_quantity")).alias("q"), F.sum(Col("l_extendedprice") * Col("l_discount")).alias("r")))

    engine.narrow_enabled = True
    on = build().collect()
    scan = engine.dev.last_scan
    assert engine._global_partial or scan["tier"] == "shared", "not a query of the private-table tier"
    assert not (scan or {}).get("narrow_slots")
    engine.narrow_enabled = False
    try:
        off = build().collect()
    finally:
        engine.narrow_enabled = True
    key = lambda r: r["l_orderkey"]  # noqa: E731
    assert sorted(on, key=key) == sorted(off, key=key) and len(on) > 10_000

    assert table.columns[3].narrow is not None  # (the table has its side forms by now)
    batch = tbl.table_batch(table, [2, 3])
    (col, _tag), = engine.dev.eval_numeric(batch, [Col("l_extendedprice") * Col("l_discount")])
    got = col.data[:ROWS].cpu().numpy()
    want = cols["l_extendedprice"].astype(np.float64) * cols["l_discount"].astype(np.float64)
    assert got.tobytes() == want.tobytes()


def test_a_narrow_column_handed_to_hs_eval_is_refused(setup):
    engine, path, table, cols = setup
    if table.columns[3].narrow is None:
        engine._encode_narrow_columns(table, [3])
    dev = engine.dev
    arr = (hs.hs_col * 1)(table.columns[3].narrow.as_hs())
    assert arr[0].kind == hs.F32_LUT8
    prog = hs.hs_program()
    out = dev.empty(ROWS, torch.float64)
    outs = (C.c_void_p * 1)(out.data_ptr())
    kinds = (C.c_int32 * 1)(hs.F64)
    rc = dev._raw_lib.hs_eval(dev.stream, arr, 1, C.byref(prog), None, ROWS, None, outs, kinds, 1, dev.flags.data_ptr())
    assert rc == 1 and b"narrow" in dev._raw_lib.hs_last_error()  # HS_E_ARG


def test_mixed_eligibility(tmp_path):
    """l_tax with 300 distinct values stays plain, the other columns go narrow; same bits as the stored columns."""
    from minispark_amd import constants, synth
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import q1
    from oracle import q1_native

    constants.SHUFFLE_FOLDER = tmp_path / "shuffle"
    with HipExecutionEngine(0) as engine:
        path = tmp_path / "lineitem.bin"
        table = synth.make_lineitem(engine.dev, path, ROWS, rows_per_block=PER_BLOCK)
        tax = ((np.arange(ROWS) * 7919) % 300).astype(np.float32) / np.float32(1000.0)
        assert len(np.unique(tax)) == 300
        table.columns[4].data.copy_(torch.from_numpy(tax))
        engine.attach_device_table(path, table)
        frame = q1(_api(engine), str(path), "1998-09-02")
        narrow = frame.collect()
        scan = engine.dev.last_scan
        assert table.columns[4].narrow is None and all(table.columns[c].narrow is not None for c in (1, 3, 6))
        assert scan["moved_bytes_per_row"] == 13 and len(scan["narrow_slots"]) == 3
        engine.narrow_enabled = False
        plain = q1(_api(engine), str(path), "1998-09-02").collect()
        assert engine.dev.last_scan["moved_bytes_per_row"] == 25
        assert narrow == plain
        cols = dict(q1_native.gen(SEED, 0, ROWS), l_tax=tax)
        assert_rows_match(narrow, _oracle(cols, table.block_rows, "1998-09-02"), max_ulps=1)


def test_the_switch_is_read_from_the_environment(monkeypatch, tmp_path):
    from minispark_amd.execution import HipExecutionEngine

    monkeypatch.setenv("HIPSPARK_NARROW", "0")
    with HipExecutionEngine(0) as engine:
        assert not engine.narrow_enabled and not engine.dev.narrow_enabled
