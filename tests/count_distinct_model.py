"""COUNT(DISTINCT e) in plain Python: the first-occurrence marks hs_mark_first must write, and the counts they add up to.

Values are compared by the token rule of tests/test_gpu_distinct.py::token: -0.0 is 0.0, every NaN is one value, bytes and
integers are themselves."""

from __future__ import annotations

import math

NAN = object()


def token(v):
    if isinstance(v, float):
        return NAN if math.isnan(v) else (0.0 if v == 0.0 else v)
    return v


def marks(columns, sel=None):
    """columns = equally long value lists (the key columns, then the argument); sel = ascending row list of the rows
    considered (None: all).  -> one 0 / 1 per input row: 1 iff the row is considered and no considered row before it holds
    the same tuple."""
    n = len(columns[0]) if columns else 0
    considered = range(n) if sel is None else sel
    first: dict = {}
    for r in considered:
        first.setdefault(tuple(token(col[r]) for col in columns), r)  # dict: the first occurrence stays
    out = [0] * n
    for r in first.values():
        out[r] = 1
    return out


def counts(keys, values, alive=None):
    """keys / values = one entry per row (a key may be a tuple, or None for the whole input); alive = one bool per row
    (None: all).  -> {key: number of different values among its living rows}; a key without a living row is absent."""
    seen: dict = {}
    for r, (k, v) in enumerate(zip(keys, values)):
        if alive is None or alive[r]:
            seen.setdefault(token(k) if not isinstance(k, tuple) else tuple(token(p) for p in k), set()).add(token(v))
    return {k: len(s) for k, s in seen.items()}
