"""Sliding window frames as plain Python: the definition ROWS BETWEEN n PRECEDING AND m FOLLOWING is tested against
(DESIGN.md 4.4i).  Partitions, order and ties are tests/window_agg_model.py's: with j a row's place in its partition's
order (ties in input order; without ORDER BY: input order) and P / L the partition's first / last place, the frame is the
places [max(P, j - n), min(L, j + m)].

``window_frame_model`` is the definition by brute force: it walks every row's frame and folds it with window_agg_model's
exact ``_Fold``.  It costs O(rows x frame).  ``window_frame_exact`` gives the same columns in O(rows log rows), for the
shapes the brute force is too slow for: sums from EXACT prefix sums (Python integers - a finite f32 times 2^149 is one - so
a difference of two prefixes is the frame's exact sum, nothing is rounded and nothing cancels; NaN and infinities are
counted, not added), MIN / MAX from a sparse table over ORDER BY's order.  tests/test_window_frames_cpu.py holds the two
against each other and the brute force against a second one written differently."""

from __future__ import annotations

import math

import numpy as np

from tests.window_agg_model import _SCALE, _Fold, _order_key, _sorted_heads

COLUMNS = ("sum", "count", "abs", "min", "max", "first", "last")


def frames_of(n: int, partition: list, order: list[tuple], preceding: int, following: int):
    """-> (perm, [(lo, hi) per SORTED place]): perm[place] = the row standing there"""
    perm, part_head, _ = _sorted_heads(n, partition, order)
    first, last = [0] * n, [0] * n
    for j in range(n):
        first[j] = j if part_head[j] else first[j - 1]
    for j in range(n - 1, -1, -1):
        last[j] = j if j + 1 == n or part_head[j + 1] else last[j + 1]
    return perm, [(max(first[j], j - preceding), min(last[j], j + following)) for j in range(n)]


def window_frame_model(n: int, partition: list, order: list[tuple], values: list, preceding: int, following: int) -> dict[str, list]:
    """partition = [values], order = [(values, ascending)], values = the argument's cells (Python ints or floats) ->
    {"sum" | "count" | "abs" | "min" | "max": one entry per row, INPUT order: the frame's exact sum, its rows, its sum of
    |x| and its least / greatest cell; "first" | "last": the ROW whose cell FIRST_VALUE / LAST_VALUE copy}."""
    is_float = any(isinstance(v, float) for v in values)
    perm, frames = frames_of(n, partition, order, preceding, following)
    out = {k: [None] * n for k in COLUMNS}
    for j, (lo, hi) in enumerate(frames):
        fold = _Fold()
        for t in range(lo, hi + 1):
            fold.add(values[perm[t]])
        row = int(perm[j])
        for k, v in fold.result(is_float).items():
            out[k][row] = v
        out["first"][row], out["last"][row] = int(perm[lo]), int(perm[hi])
    return out


def window_frame_exact(n: int, partition: list, order: list[tuple], values: list, preceding: int, following: int) -> dict[str, list]:
    """window_frame_model's columns without walking the frames."""
    is_float = any(isinstance(v, float) for v in values)
    perm, frames = frames_of(n, partition, order, preceding, following)
    cells = [values[r] for r in perm]
    finite = [not isinstance(v, float) or math.isfinite(v) for v in cells]
    scaled = [(int(math.ldexp(v, _SCALE)) if isinstance(v, float) else v) if ok else 0 for v, ok in zip(cells, finite)]

    def prefix(items):
        total, out = 0, [0]
        for v in items:
            total += v
            out.append(total)
        return out

    sums, mass = prefix(scaled), prefix(abs(v) for v in scaled)
    nan = prefix(int(isinstance(v, float) and math.isnan(v)) for v in cells)
    pinf, ninf = prefix(int(v == math.inf) for v in cells), prefix(int(v == -math.inf) for v in cells)
    # a sparse table over ranks in ORDER BY's order: level k holds the least / greatest rank of 2^k places
    keys = sorted({_order_key(v) for v in cells})
    rank_of = {k: i for i, k in enumerate(keys)}
    cell_of = {}
    for v in cells:
        cell_of.setdefault(rank_of[_order_key(v)], v)
    ranks = np.array([rank_of[_order_key(v)] for v in cells], dtype=np.int64)
    least, greatest = [ranks], [ranks]
    while 2 << (len(least) - 1) <= n:
        half = 1 << (len(least) - 1)
        least.append(np.minimum(least[-1][:-half], least[-1][half:]))
        greatest.append(np.maximum(greatest[-1][:-half], greatest[-1][half:]))
    out = {k: [None] * n for k in COLUMNS}
    for j, (lo, hi) in enumerate(frames):
        row, rows = int(perm[j]), hi - lo + 1
        between = lambda p: p[hi + 1] - p[lo]  # noqa: E731
        if not is_float:
            total = between(sums)
        elif between(nan) or (between(pinf) and between(ninf)):
            total = math.nan
        elif between(pinf) or between(ninf):
            total = math.inf if between(pinf) else -math.inf
        else:
            total = between(sums) / (1 << _SCALE)  # int / int: correctly rounded
        level = rows.bit_length() - 1
        out["sum"][row], out["count"][row] = total, rows
        weight = math.inf if between(nan) or between(pinf) or between(ninf) else between(mass)
        out["abs"][row] = float(weight) if not is_float or weight == math.inf else weight / (1 << _SCALE)
        out["min"][row] = cell_of[int(min(least[level][lo], least[level][hi + 1 - (1 << level)]))]
        out["max"][row] = cell_of[int(max(greatest[level][lo], greatest[level][hi + 1 - (1 << level)]))]
        out["first"][row], out["last"][row] = int(perm[lo]), int(perm[hi])
    return out
