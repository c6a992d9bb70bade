"""ORDER BY microbenchmark (hs_order_by), HIP events on the launch stream, median and min - max of --reps runs after warm-up:
  (a) full sort, one INTEGER key
  (b) full sort, (12-byte STRING, INTEGER DESC)
  (c) LIMIT 100 over the INTEGER key
  (d) hs_sort_by_order on the same row count with n_order = 2^31: the same four byte passes over (word, row) - the
      yardstick that existed before; (a) adds the key-forming pass and the read-backs between its steps.
hs_order_by reads a few words back between its steps, so its times include those host round trips.
Usage: python tools/bench_order_by.py [--rows 64M] [--reps 20] [--out profiles/r08_order_by_64M.txt]"""
from __future__ import annotations

import argparse
import ctypes as C
import socket
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402
from tools.bench_join_str import keys12  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=64 * 2**20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(a.rows)
    lib = hs.load_library()
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    ints = torch.randint(0, 2**31, (n,), device="cuda", generator=g, dtype=torch.int64)
    i32 = ints.to(torch.int32)
    sdata = keys12(torch.randint(0, 1 << 20, (n,), device="cuda", generator=g))  # ~64 rows per string: the INTEGER key matters
    stream = torch.cuda.current_stream().cuda_stream
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    srt = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.hs_order_by_ws_bytes(n, 2, 3)), int(lib.hs_sort_by_order_ws_bytes(n))) + 256,
                     dtype=torch.uint8, device="cuda")
    count = C.c_int64(0)
    int_key = hs.hs_col(hs.I32, -1, i32.data_ptr(), None, None)
    str_key = hs.hs_col(hs.STR, 12, sdata.data_ptr(), None, None)

    def order_by(cols, desc, limit):
        arr = (hs.hs_col * len(cols))(*cols)
        d = (C.c_int32 * len(cols))(*desc)

        def run():
            hs.check(lib.hs_order_by(stream, arr, d, len(cols), n, None, limit, perm.data_ptr(), C.byref(count),
                                     ws.data_ptr(), None), "hs_order_by")
        return run

    def sort_by_order():
        hs.check(lib.hs_sort_by_order(stream, ints.data_ptr(), n, 2**31, perm.data_ptr(), srt.data_ptr(), ws.data_ptr()),
                 "hs_sort_by_order")

    cases = [("a", "full sort, INTEGER", order_by([int_key], [0], -1)),
             ("b", "full sort, (STRING 12, INTEGER DESC)", order_by([str_key, int_key], [0, 1], -1)),
             ("c", "LIMIT 100, INTEGER", order_by([int_key], [0], 100)),
             ("d", "hs_sort_by_order, n_order 2^31", sort_by_order)]
    med = {}
    lines = [f"tools/bench_order_by.py --rows {n} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, host {socket.gethostname()}, "
             f"torch {torch.__version__}]", "events on the launch stream; median (min - max) ms, rows/s at the median"]
    for tag, what, fn in cases:
        m, lo, hi = timed(fn, a.reps)
        med[tag] = m
        lines.append(f"({tag}) {what:40s} {m:9.3f} ms ({lo:.3f} - {hi:.3f})   {n / m / 1e6:8.2f} G rows/s")
    # (a) and (c) checked against each other: the limited answer is the head of the full one
    order_by([int_key], [0], -1)()
    head = perm[:100].clone()
    order_by([int_key], [0], 100)()
    torch.cuda.synchronize()
    lines.append(f"check: LIMIT 100 equals the head of the full sort: {bool(torch.equal(head, perm[:100]))}; count = {count.value}")
    lines.append(f"(a)/(d) = {med['a'] / med['d']:.2f}    (c)/(a) = {med['c'] / med['a']:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
