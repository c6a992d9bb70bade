"""Plain Python statements of the aggregate tail of include/hipspark.h: the final fold of partial rows, the projection
after it, the rounding to stored kinds (hs_agg_finish), the rank-order merge of raw unit tables (hs_agg_units_merge),
their emission into an exchange slab (hs_agg_units_to_slab), and the general-sequence twins hs_agg_pack and
hs_slab_unpack.

Every operator here has ONE sequential order, so tests/test_gpu_agg_tail.py compares bit for bit and takes no tolerance.
Arithmetic is Python ``float`` / ``int`` (the reference is Python); numpy only holds bytes.  The models are pinned on
the CPU by tests/test_agg_tail_models.py.

Values a model cannot state - a cell whose store raises in the reference, a quotient whose divisor is zero - come back
as ``None`` next to the flag; the reference has no bytes for them, and a caller compares everything else."""

from __future__ import annotations

import struct

import numpy as np

from minispark_amd import hipspark as hs
from oracle import py_engine

MAX_INT, MIN_INT = 2**31 - 1, -(2**31)  # the reference's MIN / MAX identities
EMPTY = 0x8000000000000000              # free slot of a raw unit table
MASK56 = 2**56 - 1
MASK64 = 2**64 - 1
SUM, MIN, MAX = hs.AGG_SUM, hs.AGG_MIN, hs.AGG_MAX


# ---- 64-bit cells -------------------------------------------------------------------------------------------------
def f64_bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def bits_f64(w: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", w & MASK64))[0]


def i64_bits(v: int) -> int:
    return v & MASK64


def bits_i64(w: int) -> int:
    w &= MASK64
    return w - 2**64 if w >> 63 else w


def cell_value(w: int, is_int: bool):
    return bits_i64(w) if is_int else bits_f64(w)


def value_cell(v, is_int: bool) -> int:
    return i64_bits(v) if is_int else f64_bits(v)


# ---- the fold (hs_acc_fold) ---------------------------------------------------------------------------------------
def identity(op: int, is_int: bool):
    if op == SUM:
        return 0 if is_int else 0.0
    ident = MAX_INT if op == MIN else MIN_INT
    return ident if is_int else float(ident)


def fold(op: int, acc, x):
    """SUM adds; MIN / MAX take x only on a strict comparison, so a NaN never replaces the accumulator."""
    if op == SUM:
        return acc + x
    if op == MIN:
        return x if x < acc else acc
    return x if x > acc else acc


def fold_partials(rows, folds):
    """rows: (order, row_index, key, values) with Python float / int values, one per slab column; folds: (column, op).
    Rows with order < 0 are dropped, the rest folded per key in ascending (order, row_index).  -> {key: [merged value per
    fold]} in first-seen order; the dict keeps the FIRST key inserted, so 0.0 / -0.0 share a group under the earlier one."""
    groups: dict = {}
    for _, _, key, values in sorted((r for r in rows if r[0] >= 0), key=lambda r: (r[0], r[1])):
        acc = groups.get(key)
        if acc is None:
            acc = groups[key] = [identity(op, type(values[src]) is int) for src, op in folds]
        for j, (src, op) in enumerate(folds):
            acc[j] = fold(op, acc[j], values[src])
    return groups


# ---- projection and store -------------------------------------------------------------------------------------------
def project(groups, exprs, schema):
    """Every expression over every merged row (key, merged values ...) with the oracle's evaluator.
    -> ([values per group], flags); a ZeroDivisionError leaves None and raises HS_FLAG_DIV_ZERO."""
    fns = [py_engine.compile_expr(e, schema) for e in exprs]
    out, flags = [], 0
    for key, merged in groups.items():
        row, vals = (key, *merged), []
        for fn in fns:
            try:
                vals.append(fn(row))
            except ZeroDivisionError:
                vals.append(None)
                flags |= hs.FLAG_DIV_ZERO
        out.append(vals)
    return out, flags


def store(value, kind: int):
    """What a result or shuffle file holds for `value`, by the reference's own functions.  -> (bytes or None, flags)"""
    try:
        if kind == hs.F32:
            return struct.pack("<f", value), 0
        if kind == hs.I32:
            return value.to_bytes(4, "little", signed=True), 0
    except OverflowError:
        return None, hs.FLAG_FLT_OVERFLOW if kind == hs.F32 else hs.FLAG_INT_OVERFLOW
    if kind == hs.I64:
        return (value & MASK64).to_bytes(8, "little"), 0
    raise ValueError(f"no stored kind {kind}")


# ---- raw unit tables -------------------------------------------------------------------------------------------------
def int_key_word(value: int, unit: int) -> int:
    """Key word of an INTEGER (or table-byte) key in unit `unit`, as csrc/hs_agg_kernel.h builds it."""
    return (value & MASK64 & MASK56) | (unit << 56)


def str_key_word(text: bytes, unit: int) -> int:
    return int.from_bytes(text, "little") | (unit << 56)


def key_bytes_of_word(word: int, nbytes: int) -> bytes:
    return (word & MASK56).to_bytes(8, "little")[:nbytes]


def units_merge(rank_tables, spec, unit_cap):
    """rank_tables: per rank (keys uint64[n_units * unit_cap], cells uint64[n_units * unit_cap * n_acc]); spec: (op, is_int)
    per accumulator.  Per unit the ranks are taken in rank order: a key's cells are folded un-rounded from the identity,
    absent keys inserted.  -> ({unit: {key word: [cells]}}, {units whose union of keys exceeds unit_cap})"""
    na = len(spec)
    n_units = len(rank_tables[0][0]) // unit_cap
    merged = {u: {} for u in range(n_units)}
    for keys, cells in rank_tables:
        for u in range(n_units):
            for s in range(u * unit_cap, (u + 1) * unit_cap):
                k = int(keys[s])
                if k == EMPTY:
                    continue
                acc = merged[u].setdefault(k, [value_cell(identity(op, bool(it)), bool(it)) for op, it in spec])
                for a, (op, it) in enumerate(spec):
                    it = bool(it)
                    v = fold(op, cell_value(acc[a], it), cell_value(int(cells[s * na + a]), it))
                    if it:
                        v = bits_i64(i64_bits(v))  # 64-bit cells wrap
                    acc[a] = value_cell(v, it)
    return merged, {u for u, table in merged.items() if len(table) > unit_cap}


def units_to_slab(keys, cells, spec, desc, background=None):
    """Raw unit tables -> the bytes of the exchange slab.  desc: unit_cap, slab_rows, nbytes, order_off, key_off, key_bytes,
    acc_off[]; `background` is what the slab held before (zeros if not given).  Row r < len(keys) of an occupied slot gets
    order key r // unit_cap, the low key bytes and every cell through store(); every other row only gets order key -1.
    -> (slab bytes, flags, [(offset, length) of cells whose store raised])"""
    slab = np.zeros(desc["nbytes"], dtype=np.uint8) if background is None else np.array(background, dtype=np.uint8, copy=True)
    na, flags, undefined, unit_cap = len(spec), 0, [], desc["unit_cap"]
    order = slab[desc["order_off"]: desc["order_off"] + 8 * desc["slab_rows"]].view(np.int64)
    kb = desc["key_bytes"]
    for row in range(desc["slab_rows"]):
        k = int(keys[row]) if row < len(keys) else EMPTY
        if k == EMPTY:
            order[row] = -1
            continue
        order[row] = row // unit_cap
        at = desc["key_off"] + row * kb
        slab[at: at + kb] = np.frombuffer(key_bytes_of_word(k, kb), dtype=np.uint8)
        for a, (op, it) in enumerate(spec):
            it, w = bool(it), int(cells[row * na + a])
            if not it and op != SUM and w == f64_bits(identity(op, False)):
                flags |= hs.FLAG_TYPE_ASSERT  # the reference still holds the int identity where a float belongs
            data, f = store(cell_value(w, it), hs.I32 if it else hs.F32)
            flags |= f
            at = desc["acc_off"][a] + 4 * row
            if data is None:
                undefined.append((at, 4))
            else:
                slab[at: at + 4] = np.frombuffer(data, dtype=np.uint8)
    return slab, flags, undefined


# ---- the general-sequence twins ----------------------------------------------------------------------------------------
def pack(rep, acc, ngroups, group_cap, kinds, unit_ids=None):
    """Dense pack of slot arrays: the occupied slots (rep >= 0) of unit u, in slot order, go to rows
    [pack_start[u], pack_start[u + 1]).  -> (pack_start[n_units + 1], out_rep, [column bytes per accumulator], out_unit)"""
    n_units, na = len(ngroups), len(kinds)
    start = [0]
    for n in ngroups:
        start.append(start[-1] + int(n))
    out_rep, out_unit, cols = [], [], [bytearray() for _ in kinds]
    for u in range(n_units):
        for s in range(u * group_cap, (u + 1) * group_cap):
            if int(rep[s]) < 0:
                continue
            out_rep.append(int(rep[s]))
            out_unit.append(int(unit_ids[u]) if unit_ids is not None else u)
            for a, kind in enumerate(kinds):
                w = int(acc[s * na + a])
                cols[a] += struct.pack("<f", bits_f64(w)) if kind == hs.F32 else bits_i64(w).to_bytes(4, "little", signed=True)
    return (np.array(start, dtype=np.int64), np.array(out_rep, dtype=np.int64),
            [np.frombuffer(bytes(c), dtype=np.uint8) for c in cols], np.array(out_unit, dtype=np.int64))


def slab_unpack(gathered, world, slab_bytes, slab_rows, order_offset, col_offsets, col_row_bytes):
    """gathered: world slabs of slab_bytes ([flags u32][pad][row count i64][order keys][columns]).
    -> (flags[world], order[world * slab_rows] with -1 at or beyond a rank's count, [column bytes over world * slab_rows])"""
    g = np.asarray(gathered, dtype=np.uint8).reshape(world, slab_bytes)
    flags = np.array([int(g[r, 0:4].view(np.int32)[0]) for r in range(world)], dtype=np.int32)
    order = np.empty(world * slab_rows, dtype=np.int64)
    for r in range(world):
        count = int(g[r, 8:16].view(np.int64)[0])
        keys = g[r, order_offset: order_offset + 8 * slab_rows].view(np.int64)
        for i in range(slab_rows):
            order[r * slab_rows + i] = keys[i] if i < count else -1
    cols = [np.concatenate([g[r, off: off + rb * slab_rows] for r in range(world)])
            for off, rb in zip(col_offsets, col_row_bytes)]
    return flags, order, cols
