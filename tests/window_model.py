"""Window ranking as plain numpy: the definition ROW_NUMBER / RANK / DENSE_RANK OVER (PARTITION BY ... ORDER BY ...) is
tested against.  Equality and order are SELECT DISTINCT's and ORDER BY's: -0.0 = 0.0, every NaN one
value that sorts after +inf, strings by bytes (a prefix before its extensions, so 'ab' < 'ab\\0'), ties in input order."""

from __future__ import annotations

import numpy as np


def codes(values) -> np.ndarray:
    """One int64 per value whose order and equality are the key's: the dense rank of the value's token."""
    values = list(values) if not isinstance(values, np.ndarray) else values
    if len(values) == 0:
        return np.zeros(0, dtype=np.int64)
    if isinstance(values, np.ndarray) and values.dtype.kind in "iub":
        return values.astype(np.int64)
    if isinstance(values, np.ndarray) and values.dtype.kind == "f" or all(isinstance(v, float) for v in values):
        v = np.asarray(values, dtype=np.float64) + 0.0   # -0.0 + 0.0 = +0.0
        nan = np.isnan(v)
        _, inverse = np.unique(np.where(nan, 0.0, v), return_inverse=True)
        return np.where(nan, np.int64(len(v) + 1), inverse.astype(np.int64))  # every NaN: one value, after +inf
    if all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in values):
        return np.asarray([int(v) for v in values], dtype=np.int64)
    tokens = np.empty(len(values), dtype=object)
    tokens[:] = [v.encode("utf-8") if isinstance(v, str) else v for v in values]  # bytes, datetimes: Python's own order
    _, inverse = np.unique(tokens, return_inverse=True)
    return inverse.astype(np.int64)


def window_model(n: int, partition: list, order: list[tuple]) -> dict[str, np.ndarray]:
    """partition = [values], order = [(values, ascending)] -> {"row_number" | "rank" | "dense_rank": int64[n]}, each in
    INPUT order.  Without order keys every row of a partition is a peer of every other: row_number follows the input,
    rank and dense_rank are 1."""
    part = [codes(v) for v in partition]
    keys = part + [codes(v) if ascending else -codes(v) for v, ascending in order]
    perm = np.lexsort(tuple(reversed(keys))) if keys else np.arange(n)  # stable: ties stay in input order
    perm = perm.astype(np.int64)
    j = np.arange(n, dtype=np.int64)

    def heads(columns):
        head = np.zeros(n, dtype=bool)
        if n:
            head[0] = True
        for c in columns:
            s = c[perm]
            head[1:] |= s[1:] != s[:-1]
        return head

    part_head, peer_head = heads(part), heads(keys)
    P = np.maximum.accumulate(np.where(part_head, j, 0)) if n else j
    Q = np.maximum.accumulate(np.where(peer_head, j, 0)) if n else j
    seen = np.cumsum(peer_head)
    out = {}
    for name, sorted_values in (("row_number", j - P + 1), ("rank", Q - P + 1), ("dense_rank", seen - seen[P] + 1 if n else j)):
        col = np.zeros(n, dtype=np.int64)
        col[perm] = sorted_values
        out[name] = col
    return out
