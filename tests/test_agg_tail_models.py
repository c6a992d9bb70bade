"""The models of tests/agg_tail_models.py on hand-computed cases, without a GPU: the places where merge order, the
MIN / MAX identities, NaN, signed zero keys and the rounding to stored kinds show."""

from __future__ import annotations

import math
import struct

import numpy as np

from minispark_amd import hipspark as hs
from minispark_amd.constants import ColumnType as T
from minispark_amd.sql import Col
from tests import agg_tail_models as m


def _rows(values_by_order, key=7):
    """One partial row per (order, value): row index = position in the list."""
    return [(order, i, key, (v,)) for i, (order, v) in enumerate(values_by_order)]


def test_block_order_decides_a_cancelling_sum():
    big = float(np.float32(1e30))
    assert m.fold_partials(_rows([(0, big), (1, -big), (2, 1.0)]), [(0, m.SUM)]) == {7: [1.0]}
    assert m.fold_partials(_rows([(2, big), (0, -big), (1, 1.0)]), [(0, m.SUM)]) == {7: [0.0]}  # -big + 1.0 + big
    # equal order keys: the row index decides, and padding rows take no part
    rows = [(0, 5, 7, (1.0,)), (0, 2, 7, (big,)), (0, 3, 7, (-big,)), (-1, 0, 7, (123.0,))]
    assert m.fold_partials(rows, [(0, m.SUM)]) == {7: [1.0]}


def test_integer_partials_sum_past_int32():
    got = m.fold_partials(_rows([(0, 2**31 - 1), (1, 2**31 - 1), (2, 5)]), [(0, m.SUM), (0, m.MAX), (0, m.MIN)])
    assert got == {7: [2**32 + 3, 2**31 - 1, 5]} and all(type(v) is int for v in got[7])
    assert m.store(2**32 + 3, hs.I32) == (None, hs.FLAG_INT_OVERFLOW)
    assert m.store(2**32 + 3, hs.I64) == ((2**32 + 3).to_bytes(8, "little"), 0)
    assert m.store(-(2**31), hs.I32) == (b"\x00\x00\x00\x80", 0) and m.store(2**31, hs.I32)[1] == hs.FLAG_INT_OVERFLOW
    assert m.store(-5, hs.I64) == ((-5).to_bytes(8, "little", signed=True), 0)


def test_min_never_leaves_its_identity_over_large_values():
    got = m.fold_partials(_rows([(0, 2**31 - 1), (1, 2**31 - 1)]), [(0, m.MIN)])
    assert got == {7: [2**31 - 1]}
    got = m.fold_partials(_rows([(0, float(2**31)), (1, 3e9)]), [(0, m.MIN), (0, m.MAX)])
    assert got == {7: [float(2**31 - 1), 3e9]} and type(got[7][0]) is float
    got = m.fold_partials(_rows([(0, -3e9), (1, float(-2**31))]), [(0, m.MAX)])
    assert got == {7: [float(-2**31)]}  # MAX likewise: nothing is strictly greater than the identity


def test_nan_partial_first_or_last():
    nan = float("nan")
    for rows in ([(0, nan), (1, 2.0), (2, -3.0)], [(0, 2.0), (1, -3.0), (2, nan)]):
        s, lo, hi = m.fold_partials(_rows(rows), [(0, m.SUM), (0, m.MIN), (0, m.MAX)])[7]
        assert math.isnan(s) and lo == -3.0 and hi == 2.0  # a NaN poisons the sum and never wins a strict comparison
    only = m.fold_partials(_rows([(0, nan)]), [(0, m.MIN), (0, m.MAX)])[7]
    assert only == [float(2**31 - 1), float(-2**31)]


def test_store_rounds_to_f32_and_flags_only_finite_overflow():
    assert m.store(float(2**24 + 1), hs.F32) == (struct.pack("<f", 2.0**24), 0)  # ties to even
    assert m.store(float(2**24 + 3), hs.F32) == (struct.pack("<f", 2.0**24 + 4), 0)
    assert m.store(3.5e38, hs.F32) == (None, hs.FLAG_FLT_OVERFLOW)
    assert m.store(-3.5e38, hs.F32) == (None, hs.FLAG_FLT_OVERFLOW)
    assert m.store(float("inf"), hs.F32) == (struct.pack("<f", float("inf")), 0)
    assert m.store(3.4028235e38, hs.F32)[1] == 0
    data, flags = m.store(float("nan"), hs.F32)
    assert flags == 0 and math.isnan(struct.unpack("<f", data)[0])


def test_signed_zero_keys_are_one_group_under_the_first_key():
    rows = [(1, 0, 0.0, (1.0,)), (0, 9, -0.0, (2.0,)), (2, 1, 0.0, (4.0,)), (0, 3, 5.0, (8.0,))]
    got = m.fold_partials(rows, [(0, m.SUM)])
    assert list(got.values()) == [[8.0], [7.0]]  # first-seen order: key 5.0 (order 0, row 3), then the zeros (order 0, row 9)
    zero = [k for k in got if k == 0.0][0]
    assert math.copysign(1.0, zero) == -1.0  # order 0 comes first: its -0.0 is the key that survives
    got = m.fold_partials([(0, 0, 0.0, (1.0,)), (1, 0, -0.0, (2.0,))], [(0, m.SUM)])
    assert math.copysign(1.0, next(iter(got))) == 1.0 and list(got.values()) == [[3.0]]


def test_projection_uses_python_semantics_and_flags_a_zero_divisor():
    schema = [("k", T.INTEGER), ("s", T.FLOAT), ("c", T.INTEGER)]
    groups = {3: [7.0, 2], -4: [1.0, 0], 5: [2.5, 4]}
    vals, flags = m.project(groups, [Col("s") / Col("c"), Col("k") + Col("c"), Col("c") / Col("k")], schema)
    assert flags == hs.FLAG_DIV_ZERO
    assert vals == [[3.5, 5, 2 / 3], [None, -4, -0.0], [0.625, 9, 0.8]]
    assert m.project({3: [7.0, 2]}, [Col("s") / Col("c")], schema) == ([[3.5]], 0)


def _table(n_units, cap, na, entries):
    """entries: (unit, slot, key word, cells)"""
    keys = np.full(n_units * cap, m.EMPTY, dtype=np.uint64)
    cells = np.full(n_units * cap * na, 0xDEADBEEF, dtype=np.uint64)  # cells of free slots are never read
    for u, s, k, c in entries:
        keys[u * cap + s] = k
        cells[(u * cap + s) * na: (u * cap + s + 1) * na] = np.array(c, dtype=np.uint64)
    return keys, cells


def test_units_merge_folds_in_rank_order_and_counts_the_union():
    cap, spec = 4, [(m.SUM, 0), (m.MIN, 1)]
    kw = [m.int_key_word(v, 1) for v in (-2, 10, 11, 12, 13)]
    big = 1e30
    ranks = [
        _table(2, cap, 2, [(1, 3, kw[0], [m.f64_bits(big), m.i64_bits(9)]), (1, 0, kw[1], [m.f64_bits(1.5), m.i64_bits(2**31 + 5)])]),
        _table(2, cap, 2, [(1, 1, kw[0], [m.f64_bits(-big), m.i64_bits(-9)]), (1, 2, kw[2], [m.f64_bits(2.0), m.i64_bits(1)])]),
        _table(2, cap, 2, [(1, 0, kw[0], [m.f64_bits(1.0), m.i64_bits(4)]), (1, 3, kw[3], [m.f64_bits(3.0), m.i64_bits(0)])]),
    ]
    merged, over = m.units_merge(ranks, spec, cap)
    assert over == set() and merged[0] == {} and len(merged[1]) == cap  # the union exactly fills the unit
    assert merged[1][kw[0]] == [m.f64_bits(1.0), m.i64_bits(-9)]
    assert merged[1][kw[1]] == [m.f64_bits(1.5), m.i64_bits(2**31 - 1)]  # MIN keeps the identity
    merged, _ = m.units_merge(ranks[::-1], spec, cap)
    assert merged[1][kw[0]] == [m.f64_bits(0.0), m.i64_bits(-9)]  # 1.0 - 1e30 + 1e30
    ranks.append(_table(2, cap, 2, [(1, 1, kw[4], [m.f64_bits(0.0), m.i64_bits(0)])]))
    merged, over = m.units_merge(ranks, spec, cap)
    assert over == {1} and len(merged[1]) == cap + 1  # cap + 1 keys: the unit outgrew its table


def test_negative_integer_key_survives_the_key_word():
    for value in (-1, -2**31, -123456, 0, 2**31 - 1):
        for unit in (0, 1, 126):
            word = m.int_key_word(value, unit)
            assert word >> 56 == unit and word != m.EMPTY
            assert int.from_bytes(m.key_bytes_of_word(word, 4), "little", signed=True) == value
    assert m.key_bytes_of_word(m.str_key_word(b"ab", 3), 2) == b"ab"
    assert m.key_bytes_of_word(m.str_key_word(b"wxyz", 126), 4) == b"wxyz"
    assert m.key_bytes_of_word(m.int_key_word(200, 5), 1) == bytes([200])


def test_units_to_slab_rounds_once_and_leaves_free_rows_alone():
    cap, spec = 2, [(m.SUM, 0), (m.SUM, 1), (m.MIN, 0)]
    desc = {"unit_cap": cap, "slab_rows": 6, "nbytes": 176, "order_off": 16, "key_off": 64, "key_bytes": 4,
            "acc_off": [96, 120, 144]}
    keys, cells = _table(2, cap, 3, [
        (0, 1, m.int_key_word(-7, 0), [m.f64_bits(float(2**24 + 1)), m.i64_bits(-3), m.f64_bits(0.5)]),
        (1, 0, m.int_key_word(9, 1), [m.f64_bits(3.5e38), m.i64_bits(2**31), m.f64_bits(float(2**31 - 1))]),
    ])
    background = np.full(desc["nbytes"], 0x5A, dtype=np.uint8)
    slab, flags, undefined = m.units_to_slab(keys, cells, spec, desc, background)
    assert flags == hs.FLAG_FLT_OVERFLOW | hs.FLAG_INT_OVERFLOW | hs.FLAG_TYPE_ASSERT
    assert undefined == [(96 + 8, 4), (120 + 8, 4)]
    assert slab[16:64].view(np.int64).tolist() == [-1, 0, 1, -1, -1, -1]  # rows 4, 5 lie beyond the tables
    assert slab[64 + 4: 64 + 8].view(np.int32)[0] == -7 and slab[64 + 8: 64 + 12].view(np.int32)[0] == 9
    assert slab[96 + 4: 96 + 8].view(np.float32)[0] == np.float32(2**24) and slab[120 + 4: 120 + 8].view(np.int32)[0] == -3
    assert slab[144 + 8: 144 + 12].view(np.float32)[0] == np.float32(2**31)  # the identity, rounded like any float
    touched = np.zeros(desc["nbytes"], dtype=bool)
    touched[16:64] = True
    for row in (1, 2):
        for off in (64, 96, 120, 144):
            touched[off + 4 * row: off + 4 * row + 4] = True
    assert (slab[~touched] == 0x5A).all()


def test_pack_and_slab_unpack_on_small_inputs():
    rep = np.array([-1, 4, 7, -1, -1, -1, 2, 3, 5], dtype=np.int64)  # 3 units x 3 slots: 2, 0 and 3 groups
    acc = np.array([w for s in range(9) for w in (m.f64_bits(s + 0.5), m.i64_bits(-s))], dtype=np.uint64)
    start, out_rep, cols, unit = m.pack(rep, acc, [2, 0, 3], 3, [hs.F32, hs.I32], unit_ids=[10, 20, 30])
    assert start.tolist() == [0, 2, 2, 5] and out_rep.tolist() == [4, 7, 2, 3, 5] and unit.tolist() == [10, 10, 30, 30, 30]
    assert cols[0].view(np.float32).tolist() == [1.5, 2.5, 6.5, 7.5, 8.5] and cols[1].view(np.int32).tolist() == [-1, -2, -6, -7, -8]
    assert m.pack(rep, acc, [2, 0, 3], 3, [hs.F32, hs.I32])[3].tolist() == [0, 0, 2, 2, 2]

    rows, nbytes = 3, 16 + 24 + 8 + 16  # order keys at 16, a 1-byte column at 40 (padded to 48), a 4-byte column at 48
    g = np.zeros((2, nbytes), dtype=np.uint8)
    for r, count in enumerate([3, 1]):
        g[r, 0:4].view(np.int32)[0] = 0x20 * r
        g[r, 8:16].view(np.int64)[0] = count
        g[r, 16:40].view(np.int64)[:] = [5 + r, 6 + r, 7 + r]
        g[r, 40:43] = [1 + 10 * r, 2 + 10 * r, 3 + 10 * r]
        g[r, 48:60].view(np.int32)[:] = [-1 - r, -2 - r, -3 - r]
    flags, order, cols = m.slab_unpack(g.reshape(-1), 2, nbytes, rows, 16, [40, 48], [1, 4])
    assert flags.tolist() == [0, 0x20] and order.tolist() == [5, 6, 7, 6, -1, -1]
    assert cols[0].tolist() == [1, 2, 3, 11, 12, 13] and cols[1].view(np.int32).tolist() == [-1, -2, -3, -2, -3, -4]
