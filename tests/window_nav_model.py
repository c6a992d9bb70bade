"""Window navigation as plain Python / numpy: the definition LAG / LEAD / FIRST_VALUE / LAST_VALUE / NTILE OVER (PARTITION
BY ... ORDER BY ... [frame]) is tested against.  Partitions, order, peers and ties are
tests/window_model.py's.  The value functions COPY a cell of another row of the row's partition (or the default), so the
cells may be anything: Python values, or the bit patterns of the stored cells as unsigned integers."""

from __future__ import annotations

import numpy as np

from tests.window_model import codes

KINDS = ("lag", "lead", "first_value", "last_value", "ntile")
FRAMES = ("partition", "range", "rows")


def _ends(head: np.ndarray) -> np.ndarray:
    """E(j): the last sorted position before the next head behind j (or the last position)."""
    n = len(head)
    j = np.arange(n, dtype=np.int64)
    last = np.ones(n, dtype=bool)
    last[:-1] = head[1:]
    return np.minimum.accumulate(np.where(last, j, n)[::-1])[::-1]


def ntile_bucket(r, rows, buckets):
    """The bucket of row number r (1-based) of `rows` rows in `buckets` buckets: the first rows mod buckets of them hold
    one row more."""
    r, rows = np.asarray(r, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    s, m = rows // buckets, rows % buckets
    big = m * (s + 1)
    return np.where(r <= big, (r - 1) // (s + 1) + 1, m + (r - 1 - big) // np.maximum(s, 1) + 1)


def window_nav_plan(n: int, partition: list, order: list[tuple]):
    """What every item over one (partition, order) shares: the rows in sorted order and, per sorted position, the
    partition's first position, its last and the last peer's -> (perm, P, E_part, E_peer)."""
    part = [codes(v) for v in partition]
    keys = part + [codes(v) if ascending else -codes(v) for v, ascending in order]
    perm = (np.lexsort(tuple(reversed(keys))) if keys else np.arange(n)).astype(np.int64)  # stable: ties in input order
    j = np.arange(n, dtype=np.int64)

    def heads(columns):
        head = np.zeros(n, dtype=bool)
        head[:1] = True
        for c in columns:
            s = c[perm]
            head[1:] |= s[1:] != s[:-1]
        return head

    part_head, peer_head = heads(part), heads(keys)
    P = np.maximum.accumulate(np.where(part_head, j, 0)) if n else j
    return perm, P, _ends(part_head), _ends(peer_head)


def window_nav_model(n: int, partition: list, order: list[tuple], cells, kind: str, frame: str | None = None,
                     k: int | None = None, default=None, buckets: int | None = None, plan=None):
    """partition = [values], order = [(values, ascending)], cells = the argument's cells (None for "ntile") -> one entry
    per row, INPUT order: an ndarray of the cells' dtype when `cells` is one, else a list.  `frame` ("partition" | "range"
    | "rows") is read for "first_value" / "last_value", `k` and `default` for "lag" / "lead", `buckets` for "ntile".
    `plan`: window_nav_plan of the same keys, for callers with many items over them."""
    assert kind in KINDS
    perm, P, E_part, E_peer = plan if plan is not None else window_nav_plan(n, partition, order)
    j = np.arange(n, dtype=np.int64)
    if kind == "ntile":
        out = np.zeros(n, dtype=np.int64)
        out[perm] = ntile_bucket(j - P + 1, E_part - P + 1, buckets)
        return out
    as_array = isinstance(cells, np.ndarray)
    if not as_array:
        held = np.empty(n, dtype=object)
        held[:] = list(cells)
        cells = held
    valid = np.ones(n, dtype=bool)
    if kind == "lag":
        s = j - k
        valid = s >= P
    elif kind == "lead":
        s = j + k
        valid = s <= E_part
    elif kind == "first_value":
        s = P
    else:
        assert frame in FRAMES
        s = j if frame == "rows" else E_peer if frame == "range" else E_part
    in_order = cells[perm]
    picked = in_order[np.clip(s, 0, max(n - 1, 0))] if n else in_order
    if not valid.all():
        picked = picked.copy()
        picked[~valid] = default
    out = np.empty(n, dtype=cells.dtype)
    out[perm] = picked
    return out if as_array else out.tolist()


def brute_force(n: int, partition: list, order: list[tuple], cells, kind: str, frame: str | None = None,
                k: int | None = None, default=None, buckets: int | None = None) -> list:
    """The same straight from the definition, row by row: list the rows of the row's partition in the window's order
    (ties in input order), find the row in it, and step."""
    part = [codes(v) for v in partition]
    keys = [codes(v) if ascending else -codes(v) for v, ascending in order]
    out = []
    for i in range(n):
        rows = [r for r in range(n) if all(p[r] == p[i] for p in part)]
        rows.sort(key=lambda r: (tuple(c[r] for c in keys), r))
        at = rows.index(i)
        mine = tuple(c[i] for c in keys)
        if kind == "ntile":
            sizes = [len(rows) // buckets + (b < len(rows) % buckets) for b in range(buckets)] if buckets <= len(rows) \
                else [1] * len(rows)
            bucket, left = 0, at
            while left >= sizes[bucket]:
                left -= sizes[bucket]
                bucket += 1
            out.append(bucket + 1)
        elif kind == "lag":
            out.append(cells[rows[at - k]] if at - k >= 0 else default)
        elif kind == "lead":
            out.append(cells[rows[at + k]] if at + k < len(rows) else default)
        elif kind == "first_value":
            out.append(cells[rows[0]])
        elif frame == "rows":
            out.append(cells[i])
        elif frame == "range":
            out.append(cells[[r for r in rows if tuple(c[r] for c in keys) == mine][-1]])
        else:
            out.append(cells[rows[-1]])
    return out
