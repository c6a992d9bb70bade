"""The four window entries at the C ABI (hs_window, hs_window_agg, hs_window_nav, hs_window_frames): one harness.  The
harnesses the test modules import from each other (tests/test_gpu_window*.py) pick the entry and the view of the cells."""

from __future__ import annotations

import ctypes as C

import numpy as np

FRAME = {"partition": 0, "range": 1, "rows": 2, "between": 3}
LAG, LAST_VALUE = 8, 11  # the functions whose column has the argument's cells: 8 bytes for a TIMESTAMP
SENTINEL, SLACK = -7, 16
# how many of the item arrays an entry takes: functions | frames, values | params, defaults | preceding, following
ENTRIES = {"hs_window": 1, "hs_window_agg": 3, "hs_window_nav": 5, "hs_window_frames": 7}


def call_window(dev, entry, cols, descending, n_part, items, n, n_keys=None, omit=()):
    """The entry point itself.  items = [(function, frame name / code or None, value column or None, k or n, default bits,
    n PRECEDING, m FOLLOWING)], fields at the end may be left out; `omit` names the arrays to pass as null: "params",
    "defaults", "preceding", "following" -> (return code, [one array per item, input order: the cells' bits as uint32,
    uint64 for an 8-byte argument], the status word).  Every output is allocated with a sentinel and SLACK cells behind
    the rows, which must stay untouched."""
    import torch

    from minispark_amd import hipspark as hs

    lib = dev._raw_lib
    n_keys = len(cols) if n_keys is None else n_keys
    field = lambda it, k: it[k] if len(it) > k else None  # noqa: E731
    ints = lambda ctype, k: (ctype * len(items))(*[int(field(it, k) or 0) for it in items])  # noqa: E731
    arr = (hs.hs_col * max(len(cols), 1))(*[c.as_hs() for c in cols])
    desc = (C.c_int32 * max(n_keys, 1))(*[int(d) for d in descending])
    frames = (C.c_int32 * len(items))(*[FRAME.get(field(it, 1), 0) if isinstance(field(it, 1), (str, type(None))) else it[1]
                                        for it in items])
    values = (hs.hs_col * len(items))(*[field(it, 2).as_hs() if field(it, 2) is not None else hs.hs_col() for it in items])
    arrays = {"functions": ints(C.c_int32, 0), "frames": frames, "values": values, "params": ints(C.c_int64, 3),
              "defaults": ints(C.c_uint64, 4), "preceding": ints(C.c_int64, 5), "following": ints(C.c_int64, 6)}
    assert set(omit) <= set(arrays)
    taken = [None if name in omit else array for name, array in arrays.items()][:ENTRIES[entry]]
    wide = [LAG <= it[0] <= LAST_VALUE and field(it, 2) is not None and field(it, 2).kind == hs.I64 for it in items]
    outs = [torch.full((n + SLACK,), SENTINEL, dtype=torch.int64 if w else torch.int32, device=dev.device) for w in wide]
    ptrs = (C.c_void_p * len(items))(*[o.data_ptr() for o in outs])
    flags = torch.zeros(2, dtype=torch.int32, device=dev.device)
    sized = (n, n_keys, 32 * max(n_keys, 1)) if entry == "hs_window" else (n, n_keys, 32 * max(n_keys, 1), len(items))
    ws = torch.empty(int(getattr(lib, entry + "_ws_bytes")(*sized)) + 256, dtype=torch.uint8, device=dev.device)
    rc = getattr(lib, entry)(dev.stream, arr, desc, n_part, n_keys, n, *taken, len(items), ptrs, ws.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    got = []
    for w, o in zip(wide, outs):
        host = o.cpu().numpy()
        assert np.all(host[n:] == SENTINEL), "cells behind the rows were written"
        got.append(host[:n].view(np.uint64 if w else np.uint32))
    return rc, got, int(flags[0].item())
