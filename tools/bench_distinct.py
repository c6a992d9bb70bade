"""SELECT DISTINCT microbenchmark (hs_distinct), HIP events on the launch stream, median and min - max of --reps runs after
warm-up.  Every case is timed next to hs_order_by without a limit over the same keys: the sort is shared, so that is the
floor, and hs_distinct adds one gather-and-compare pass (k_distinct_heads) and one compaction (hs_compact):
  (a) one INTEGER column, about --distinct different values
  (b) one INTEGER column, every value different
  (c) a two-word key: (TIMESTAMP, INTEGER), about --distinct different rows
(a) and (b) are keys of one word: hs_distinct then compares the sorted words the sort left behind; with
HIPSPARK_DISTINCT_GATHER=1 it forms the words again from the columns as it does for longer keys - both are timed.
Both calls read a few words back between their steps, so their times include those host round trips.
Usage: python tools/bench_distinct.py [--rows 64M] [--distinct 1M] [--reps 20] [--out profiles/r10_distinct.txt]"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import socket
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402
from tools.bench_order_by import timed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=64 * 2**20)
    ap.add_argument("--distinct", type=float, default=2**20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d = int(a.rows), int(a.distinct)
    lib = hs.load_library()
    g = torch.Generator(device="cuda")
    g.manual_seed(10)
    few = torch.randint(0, d, (n,), device="cuda", generator=g, dtype=torch.int64)
    few32 = few.to(torch.int32)
    unique32 = torch.randperm(n, device="cuda", generator=g).to(torch.int32)
    stamps = few * 1_000_003 + 1_700_000_000  # one stamp per value of `few`: the pair has as many different rows
    stream = torch.cuda.current_stream().cuda_stream
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.hs_distinct_ws_bytes(n, 2, 3)) + 256, dtype=torch.uint8, device="cuda")
    count = C.c_int64(0)
    col = lambda kind, t: hs.hs_col(kind, -1, t.data_ptr(), None, None)  # noqa: E731
    cases = [("a", f"INTEGER, ~{d} values", [col(hs.I32, few32)]),
             ("b", "INTEGER, all different", [col(hs.I32, unique32)]),
             ("c", f"(TIMESTAMP, INTEGER), ~{d} rows", [col(hs.I64, stamps), col(hs.I32, few32)])]

    def distinct(cols):
        arr = (hs.hs_col * len(cols))(*cols)

        def run():
            hs.check(lib.hs_distinct(stream, arr, len(cols), n, None, perm.data_ptr(), C.byref(count), ws.data_ptr(), None),
                     "hs_distinct")
        return run

    def order_by(cols):
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))

        def run():
            hs.check(lib.hs_order_by(stream, arr, asc, len(cols), n, None, -1, perm.data_ptr(), C.byref(count), ws.data_ptr(),
                                     None), "hs_order_by")
        return run

    lines = [f"tools/bench_distinct.py --rows {n} --distinct {d} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, host "
             f"{socket.gethostname()}, torch {torch.__version__}]",
             "events on the launch stream; median (min - max) ms, rows/s at the median; ratio = hs_distinct / hs_order_by"]
    for tag, what, cols in cases:
        md, lo, hi = timed(distinct(cols), a.reps)
        kept = count.value
        lines.append(f"({tag}) hs_distinct  {what:34s} {md:9.3f} ms ({lo:.3f} - {hi:.3f})   {n / md / 1e6:8.2f} G rows/s   "
                     f"{kept} rows survive")
        if len(cols) == 1:  # the general path on the same key
            os.environ["HIPSPARK_DISTINCT_GATHER"] = "1"
            mg, lo, hi = timed(distinct(cols), a.reps)
            del os.environ["HIPSPARK_DISTINCT_GATHER"]
            lines.append(f"({tag}) hs_distinct  {'  words formed again (GATHER=1)':34s} {mg:9.3f} ms ({lo:.3f} - {hi:.3f})   "
                         f"{n / mg / 1e6:8.2f} G rows/s   {count.value} rows survive")
        ms, lo, hi = timed(order_by(cols), a.reps)
        lines.append(f"({tag}) hs_order_by  {what:34s} {ms:9.3f} ms ({lo:.3f} - {hi:.3f})   {n / ms / 1e6:8.2f} G rows/s   "
                     f"ratio {md / ms:.2f}")
    # (a) checked: the survivors are ascending, as many as there are values, and every one is its value's first row
    distinct(cases[0][2])()
    torch.cuda.synchronize()
    kept = perm[:count.value]
    first = torch.full((d,), n, dtype=torch.int64, device="cuda").scatter_reduce(0, few, torch.arange(n, device="cuda"), "amin")
    ok = bool((kept[1:] > kept[:-1]).all()) and bool(torch.equal(kept, first[first < n].sort().values))
    lines.append(f"check (a): the survivors are the first row of every value, ascending: {ok}; count = {count.value}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
