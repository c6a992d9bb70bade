"""Window aggregates as plain Python / numpy: the definition SUM / AVG / MIN / MAX / COUNT OVER (PARTITION BY ... ORDER BY
... frame) is tested against.  Partitions, order, peers and ties are tests/window_model.py's.  A frame is
"partition" (every row of the row's partition), "range" (the partition's first row through the row's LAST peer) or "rows"
(through the row itself, ties in input order).  Sums are EXACT: Python ints for INTEGER, for FLOAT the correctly rounded
f64 of the exact sum (what math.fsum returns), NaN / infinities as IEEE adds them.  MIN / MAX compare in ORDER BY's order:
-0.0 = 0.0, NaN after +inf."""

from __future__ import annotations

import math

import numpy as np

from tests.window_model import codes

FRAMES = ("partition", "range", "rows")
_SCALE = 149  # a finite f32 times 2^149 is an integer


def _order_key(v):
    """ORDER BY's total order on one cell: NaN after +inf, the two zeros one value."""
    if isinstance(v, float):
        return (1, 0.0) if math.isnan(v) else (0, v + 0.0)
    return (0, v)


class _Fold:
    """The exact fold of the cells added so far."""

    def __init__(self):
        self.count, self.ints, self.abs, self.nan, self.pinf, self.ninf, self.lo, self.hi = 0, 0, 0.0, 0, 0, 0, None, None

    def add(self, v):
        self.count += 1
        if isinstance(v, float):
            if math.isnan(v):
                self.nan += 1
            elif math.isinf(v):
                self.pinf += v > 0
                self.ninf += v < 0
            else:
                self.ints += int(math.ldexp(v, _SCALE))
            self.abs += abs(v)
        else:
            self.ints += v
            self.abs += float(abs(v))
        if self.lo is None or _order_key(v) < _order_key(self.lo):
            self.lo = v
        if self.hi is None or _order_key(v) > _order_key(self.hi):
            self.hi = v

    def result(self, is_float):
        if not is_float:
            total = self.ints
        elif self.nan or (self.pinf and self.ninf):
            total = math.nan
        elif self.pinf or self.ninf:
            total = math.inf if self.pinf else -math.inf
        else:
            total = self.ints / (1 << _SCALE)  # int / int: correctly rounded
        return {"sum": total, "count": self.count, "abs": self.abs, "min": self.lo, "max": self.hi}


def _sorted_heads(n, partition, order):
    part = [codes(v) for v in partition]
    keys = part + [codes(v) if ascending else -codes(v) for v, ascending in order]
    perm = (np.lexsort(tuple(reversed(keys))) if keys else np.arange(n)).astype(np.int64)  # stable: ties in input order

    def heads(columns):
        head = np.zeros(n, dtype=bool)
        head[:1] = True
        for c in columns:
            s = c[perm]
            head[1:] |= s[1:] != s[:-1]
        return head

    return perm, heads(part), heads(keys)


def window_agg_model(n: int, partition: list, order: list[tuple], values: list, frame: str) -> dict[str, list]:
    """partition = [values], order = [(values, ascending)], values = the argument's cells (Python ints or floats) ->
    {"sum" | "count" | "abs" | "min" | "max": one entry per row, INPUT order}: the frame's exact sum, its rows, its sum of
    |x| (f64, for error bounds) and its least / greatest cell."""
    assert frame in FRAMES
    is_float = any(isinstance(v, float) for v in values)
    perm, part_head, peer_head = _sorted_heads(n, partition, order)
    running, fold = [], None
    for j in range(n):  # the fold over [P(j), j]
        if part_head[j]:
            fold = _Fold()
        fold.add(values[perm[j]])
        running.append(fold.result(is_float))
    end_head = peer_head if frame == "range" else part_head
    out = {k: [None] * n for k in ("sum", "count", "abs", "min", "max")}
    end = n - 1
    for j in range(n - 1, -1, -1):  # E(j): the last position before the next run of peers / the next partition
        if frame == "rows":
            end = j
        elif j + 1 < n and end_head[j + 1]:
            end = j
        for k, column in out.items():
            column[perm[j]] = running[end][k]
    return out


def brute_force(n: int, partition: list, order: list[tuple], values: list, frame: str) -> dict[str, list]:
    """The same straight from the definition: for every row, list the rows of its frame and fold them."""
    part = [codes(v) for v in partition]
    keys = [codes(v) if ascending else -codes(v) for v, ascending in order]
    is_float = any(isinstance(v, float) for v in values)
    out = {k: [] for k in ("sum", "count", "abs", "min", "max")}
    for i in range(n):
        mine = tuple(k[i] for k in keys)
        rows = []
        for r in range(n):
            if any(p[r] != p[i] for p in part):
                continue
            theirs = tuple(k[r] for k in keys)
            if frame == "partition" or theirs < mine or (theirs == mine and (frame == "range" or r <= i)):
                rows.append(r)
        cells = [values[r] for r in rows]
        out["sum"].append(math.fsum(cells) if is_float and all(math.isfinite(c) for c in cells)
                          else sum(cells) if not is_float else _nonfinite_sum(cells))
        out["count"].append(len(cells))
        out["abs"].append(math.fsum(abs(c) for c in cells) if is_float else float(sum(abs(c) for c in cells)))
        out["min"].append(min(cells, key=_order_key))
        out["max"].append(max(cells, key=_order_key))
    return out


def _nonfinite_sum(cells):
    if any(math.isnan(c) for c in cells) or (math.inf in cells and -math.inf in cells):
        return math.nan
    return math.inf if math.inf in cells else -math.inf


def same(a, b) -> bool:
    """Equal as values: NaN is NaN, the two zeros are one."""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b
