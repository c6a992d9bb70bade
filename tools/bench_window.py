"""Window ranking microbenchmark (hs_window), HIP events on the launch stream, median and min - max of --reps runs after
warm-up.  Every case is timed next to hs_order_by without a limit over the same keys, the two alternating run by run:
the sort is shared, so that is the floor, and hs_window adds the heads pass, the three scan passes and one 4-byte scatter
per function:
  (a) PARTITION BY an INTEGER with about --partitions values ORDER BY an INTEGER, ROW_NUMBER only (one key word)
  (b) the same, ROW_NUMBER + RANK + DENSE_RANK
  (c) PARTITION BY a TIMESTAMP ORDER BY an INTEGER, all three (two key words: the words are formed again)
  (d) no PARTITION BY, ORDER BY an INTEGER, all three
Window aggregates (hs_window_agg), over case (a)'s keys, each timed next to hs_window ROW_NUMBER on the same keys (the cheapest
windowed call there is: the aggregate adds a 4-byte gather of its argument, its scan passes and, like ROW_NUMBER, one scatter):
  (e) SUM(INTEGER), default frame (RANGE: through the last peer)
  (f) SUM(FLOAT) over the whole partition
  (g) SUM(FLOAT), ROWS frame
  (h) ROW_NUMBER + RANK + DENSE_RANK + SUM(INTEGER) + COUNT in one call, default frame
Window navigation (hs_window_nav), over case (a)'s keys, each timed next to hs_window ROW_NUMBER on the same keys like (e) - (h)
(a value item adds one gather of its argument into sorted order and one scatter; LEAD / NTILE / LAST_VALUE one end-table pass):
  (i) LAG(INTEGER, 1)
  (j) LEAD(TIMESTAMP, 1): 8-byte cells
  (k) LAST_VALUE(FLOAT), default frame (RANGE: the last peer)
  (l) ROW_NUMBER + SUM(INTEGER) + LAG(INTEGER, 1) + NTILE(4) in one call, default frame
Sliding frames (hs_window_frames), SUM(FLOAT) ROWS BETWEEN n PRECEDING AND n FOLLOWING, each timed next to
hs_window ROW_NUMBER on the same keys (a sliding item adds the block heads, one gather, a forward and a backward scan with
their tile carries, and one scatter that reads two tables); the cost must not depend on n:
  (m) n = 1   (n) n = 500   (o) n = 50 000       over case (a)'s keys: partitions of about 64 rows clamp the wider frames
  (p) n = 1   (q) n = 500   (r) n = 50 000       over case (d)'s key: ONE partition, every frame as wide as it says
Both calls read a few words back between their steps, so their times include those host round trips.  --case x --reps 3
under a kernel trace gives the per-kernel split.  --lib PATH times another build of the library (the parent commit's, for
"ranking did not move"); a library without hs_window_agg runs (a) - (d) only, one without hs_window_nav (a) - (h), one
without hs_window_frames (a) - (l).
Usage: python tools/bench_window.py [--rows 64M] [--partitions 1M] [--reps 20] [--case abcdefghijklmnopqr] [--lib libhipspark.so]
                                    [--out profiles/r21_window_nav.txt]"""
from __future__ import annotations

import argparse
import ctypes as C
import socket
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402


def timed_pair(first, second, reps):
    """Both functions alternating, run by run -> (median, min, max) ms of each."""
    for _ in range(2):
        first()
        second()
    torch.cuda.synchronize()
    times = ([], [])
    for _ in range(reps):
        for fn, ts in zip((first, second), times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
    return [(sorted(ts)[len(ts) // 2], min(ts), max(ts)) for ts in times]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=64 * 2**20)
    ap.add_argument("--partitions", type=float, default=2**20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", default="abcdefghijklmnopqr")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d = int(a.rows), int(a.partitions)
    if a.lib:  # another build: bind what it exports
        lib = C.CDLL(str(Path(a.lib).resolve()))
        for name, (restype, argtypes) in hs.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    else:
        lib = hs.load_library()
    has_agg = hasattr(lib, "hs_window_agg")
    has_nav = hasattr(lib, "hs_window_nav")
    has_frames = hasattr(lib, "hs_window_frames")
    a.case = "".join(tag for tag in a.case if tag in "abcd" or (has_agg and tag in "efgh") or (has_nav and tag in "ijkl") or has_frames)
    g = torch.Generator(device="cuda")
    g.manual_seed(15)
    part = torch.randint(0, d, (n,), device="cuda", generator=g, dtype=torch.int64)
    part32 = part.to(torch.int32)
    order32 = torch.randint(0, 1000, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    stamps = part * 1_000_003 + 1_700_000_000
    stream = torch.cuda.current_stream().cuda_stream
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    outs = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(5 if has_agg else 3)]
    ws_bytes = (lib.hs_window_frames_ws_bytes(n, 2, 3, 5) if has_frames else lib.hs_window_nav_ws_bytes(n, 2, 3, 5) if has_nav else lib.hs_window_agg_ws_bytes(n, 2, 3, 5) if has_agg
                else lib.hs_window_ws_bytes(n, 2, 3))
    ws = torch.empty(int(ws_bytes) + 256, dtype=torch.uint8, device="cuda")
    count = C.c_int64(0)
    col = lambda kind, t: hs.hs_col(kind, -1, t.data_ptr(), None, None)  # noqa: E731
    every = [hs.WIN_ROW_NUMBER, hs.WIN_RANK, hs.WIN_DENSE_RANK]
    cases = {"a": ("(INTEGER | INTEGER), ROW_NUMBER", [col(hs.I32, part32), col(hs.I32, order32)], 1, every[:1]),
             "b": ("(INTEGER | INTEGER), all three", [col(hs.I32, part32), col(hs.I32, order32)], 1, every),
             "c": ("(TIMESTAMP | INTEGER), all three", [col(hs.I64, stamps), col(hs.I32, order32)], 1, every),
             "d": ("( | INTEGER), all three", [col(hs.I32, order32)], 0, every)}

    def window(cols, n_part, funcs):
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))
        kinds = (C.c_int32 * len(funcs))(*funcs)
        ptrs = (C.c_void_p * len(funcs))(*[o.data_ptr() for o in outs[:len(funcs)]])

        def run():
            hs.check(lib.hs_window(stream, arr, asc, n_part, len(cols), n, kinds, len(funcs), ptrs, ws.data_ptr(), None), "hs_window")
        return run

    def order_by(cols):
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))

        def run():
            hs.check(lib.hs_order_by(stream, arr, asc, len(cols), n, None, -1, perm.data_ptr(), C.byref(count), ws.data_ptr(),
                                     None), "hs_order_by")
        return run

    def window_agg(cols, n_part, items):
        """items = [(function, frame, argument column or None)]"""
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))
        kinds = (C.c_int32 * len(items))(*[f for f, _, _ in items])
        frames = (C.c_int32 * len(items))(*[fr for _, fr, _ in items])
        values = (hs.hs_col * len(items))(*[v if v is not None else hs.hs_col() for _, _, v in items])
        ptrs = (C.c_void_p * len(items))(*[o.data_ptr() for o in outs[:len(items)]])

        def run():
            hs.check(lib.hs_window_agg(stream, arr, asc, n_part, len(cols), n, kinds, frames, values, len(items), ptrs,
                                       ws.data_ptr(), flags.data_ptr()), "hs_window_agg")
        return run

    agg_cases = {}
    if has_agg:
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        ints = torch.randint(-1000, 1001, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
        floats = torch.rand(n, device="cuda", generator=g, dtype=torch.float32) * 2000.0 - 1000.0
        vi, vf = col(hs.I32, ints), col(hs.F32, floats)
        agg_cases = {"e": ("SUM(INTEGER), default frame", [(hs.WIN_SUM, hs.WIN_FRAME_RANGE, vi)]),
                     "f": ("SUM(FLOAT), whole partition", [(hs.WIN_SUM, hs.WIN_FRAME_PARTITION, vf)]),
                     "g": ("SUM(FLOAT), ROWS", [(hs.WIN_SUM, hs.WIN_FRAME_ROWS, vf)]),
                     "h": ("three ranks + SUM(INTEGER) + COUNT", [(hs.WIN_ROW_NUMBER, 0, None), (hs.WIN_RANK, 0, None),
                                                                  (hs.WIN_DENSE_RANK, 0, None), (hs.WIN_SUM, hs.WIN_FRAME_RANGE, vi),
                                                                  (hs.WIN_COUNT, hs.WIN_FRAME_RANGE, None)])}

    def window_nav(cols, n_part, items):
        """items = [(function, frame, argument column or None, k or n)]; the default cell is 0"""
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))
        kinds = (C.c_int32 * len(items))(*[it[0] for it in items])
        frames = (C.c_int32 * len(items))(*[it[1] for it in items])
        values = (hs.hs_col * len(items))(*[it[2] if it[2] is not None else hs.hs_col() for it in items])
        params = (C.c_int64 * len(items))(*[it[3] for it in items])
        defaults = (C.c_uint64 * len(items))()
        ptrs = (C.c_void_p * len(items))(*[(wide_out if it[2] is not None and it[2].kind == hs.I64 else o).data_ptr()
                                           for it, o in zip(items, outs)])

        def run():
            hs.check(lib.hs_window_nav(stream, arr, asc, n_part, len(cols), n, kinds, frames, values, params, defaults, len(items),
                                       ptrs, ws.data_ptr(), flags.data_ptr()), "hs_window_nav")
        return run

    nav_cases = {}
    if has_nav:
        wide_out = torch.empty(n, dtype=torch.int64, device="cuda")
        vt = col(hs.I64, stamps)
        nav_cases = {"i": ("LAG(INTEGER, 1)", [(hs.WIN_LAG, 0, vi, 1)]),
                     "j": ("LEAD(TIMESTAMP, 1)", [(hs.WIN_LEAD, 0, vt, 1)]),
                     "k": ("LAST_VALUE(FLOAT), default frame", [(hs.WIN_LAST_VALUE, hs.WIN_FRAME_RANGE, vf, 0)]),
                     "l": ("ROW_NUMBER + SUM(INTEGER) + LAG + NTILE(4)", [(hs.WIN_ROW_NUMBER, 0, None, 0),
                                                                          (hs.WIN_SUM, hs.WIN_FRAME_RANGE, vi, 0),
                                                                          (hs.WIN_LAG, 0, vi, 1), (hs.WIN_NTILE, 0, None, 4)])}

    def window_frames(cols, n_part, items):
        """items = [(function, argument column, n PRECEDING, m FOLLOWING)], all of HS_WIN_FRAME_BETWEEN"""
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))
        kinds = (C.c_int32 * len(items))(*[it[0] for it in items])
        frames = (C.c_int32 * len(items))(*[hs.WIN_FRAME_BETWEEN] * len(items))
        values = (hs.hs_col * len(items))(*[it[1] for it in items])
        before, after = (C.c_int64 * len(items))(*[it[2] for it in items]), (C.c_int64 * len(items))(*[it[3] for it in items])
        ptrs = (C.c_void_p * len(items))(*[o.data_ptr() for o in outs[:len(items)]])

        def run():
            hs.check(lib.hs_window_frames(stream, arr, asc, n_part, len(cols), n, kinds, frames, values, None, None, before, after,
                                          len(items), ptrs, ws.data_ptr(), flags.data_ptr()), "hs_window_frames")
        return run

    frame_cases = {}
    if has_frames:
        frame_cases = {tag: (f"SUM(FLOAT), ({k}, {k}), keys of ({keys})", keys, [(hs.WIN_SUM, vf, k, k)])
                       for tag, keys, k in (("m", "a", 1), ("n", "a", 500), ("o", "a", 50000), ("p", "d", 1), ("q", "d", 500),
                                            ("r", "d", 50000))}

    lines = [f"tools/bench_window.py --rows {n} --partitions {d} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, host "
             f"{socket.gethostname()}, torch {torch.__version__}]",
             "events on the launch stream, the two calls alternating; median (min - max) ms; ratio = hs_window / hs_order_by"]
    for tag in a.case:
        if tag in frame_cases:
            what, keys, items = frame_cases[tag]
            _, cols, n_part, _ = cases[keys]
            (mw, lw, hw), (ms, lo, hi) = timed_pair(window_frames(cols, n_part, items), window(cols, n_part, every[:1]), a.reps)
            lines.append(f"({tag}) hs_window_frames {what:30s} {mw:9.3f} ms ({lw:.3f} - {hw:.3f})   {n / mw / 1e6:8.2f} G rows/s")
            lines.append(f"({tag}) hs_window    {'the same keys, ROW_NUMBER':34s} {ms:9.3f} ms ({lo:.3f} - {hi:.3f})   "
                         f"{n / ms / 1e6:8.2f} G rows/s   ratio {mw / ms:.2f}   + {mw - ms:.3f} ms")
            continue
        if tag in agg_cases or tag in nav_cases:
            what, items = agg_cases[tag] if tag in agg_cases else nav_cases[tag]
            entry, call = ("hs_window_agg", window_agg) if tag in agg_cases else ("hs_window_nav", window_nav)
            _, cols, n_part, _ = cases["a"]
            (mw, lw, hw), (ms, lo, hi) = timed_pair(call(cols, n_part, items), window(cols, n_part, every[:1]), a.reps)
            lines.append(f"({tag}) {entry} {what:33s} {mw:9.3f} ms ({lw:.3f} - {hw:.3f})   {n / mw / 1e6:8.2f} G rows/s")
            lines.append(f"({tag}) hs_window    {'the same keys, ROW_NUMBER':34s} {ms:9.3f} ms ({lo:.3f} - {hi:.3f})   "
                         f"{n / ms / 1e6:8.2f} G rows/s   ratio {mw / ms:.2f}   + {mw - ms:.3f} ms")
            continue
        what, cols, n_part, funcs = cases[tag]
        (mw, lw, hw), (ms, lo, hi) = timed_pair(window(cols, n_part, funcs), order_by(cols), a.reps)
        lines.append(f"({tag}) hs_window    {what:34s} {mw:9.3f} ms ({lw:.3f} - {hw:.3f})   {n / mw / 1e6:8.2f} G rows/s")
        lines.append(f"({tag}) hs_order_by  {'the same keys, no limit':34s} {ms:9.3f} ms ({lo:.3f} - {hi:.3f})   "
                     f"{n / ms / 1e6:8.2f} G rows/s   ratio {mw / ms:.2f}   + {mw - ms:.3f} ms")
    if "b" in a.case:  # checked against the sort's own row list: row_number restarts with the partition, rank <= row_number
        what, cols, n_part, funcs = cases["b"]
        window(cols, n_part, funcs)()
        order_by(cols)()
        torch.cuda.synchronize()
        rn, rk, dr = (o[perm].to(torch.int64) for o in outs[:3])
        p, o = part32[perm], order32[perm]
        new_part = torch.ones(n, dtype=torch.bool, device="cuda")
        new_part[1:] = p[1:] != p[:-1]
        new_peer = new_part.clone()
        new_peer[1:] |= o[1:] != o[:-1]
        ok = (bool((rn[new_part] == 1).all()) and bool((rn[1:][~new_part[1:]] == rn[:-1][~new_part[1:]] + 1).all())
              and bool((rk[new_peer] == rn[new_peer]).all()) and bool((rk[1:][~new_peer[1:]] == rk[:-1][~new_peer[1:]]).all())
              and bool((dr[new_part] == 1).all())
              and bool((dr[1:][~new_part[1:]] == dr[:-1][~new_part[1:]] + new_peer[1:][~new_part[1:]].to(torch.int64)).all()))
        lines.append(f"check (b): along the sorted rows row_number counts up inside a partition, rank is the row_number of the "
                     f"first peer, dense_rank steps by one per group of peers: {ok}")
    if "e" in a.case:  # checked with torch over the sort's own row list: the running sum through the last peer
        what, items = agg_cases["e"]
        _, cols, n_part, _ = cases["a"]
        window_agg(cols, n_part, items)()
        order_by(cols)()
        torch.cuda.synchronize()
        p, o, v = part32[perm].to(torch.int64), order32[perm].to(torch.int64), ints[perm].to(torch.int64)
        prefix = torch.cumsum(v, 0)
        position = torch.arange(n, device="cuda")
        new_part = torch.ones(n, dtype=torch.bool, device="cuda")
        new_part[1:] = p[1:] != p[:-1]
        last_peer = torch.ones(n, dtype=torch.bool, device="cuda")
        last_peer[:-1] = (p[1:] != p[:-1]) | (o[1:] != o[:-1])
        start = torch.cummax(torch.where(new_part, position, torch.zeros_like(position)), 0).values
        end = torch.flip(torch.cummin(torch.flip(torch.where(last_peer, position, torch.full_like(position, n)), [0]), 0).values, [0])
        want = prefix[end] - prefix[start] + v[start]
        ok = bool((outs[0][perm].to(torch.int64) == want).all()) and int(flags[0].item()) == 0
        lines.append(f"check (e): along the sorted rows the sum is the partition's prefix sum at the row's last peer: {ok}")
    if "i" in a.case:  # checked with torch over the sort's own row list: the left neighbour's cell inside a partition
        what, items = nav_cases["i"]
        _, cols, n_part, _ = cases["a"]
        window_nav(cols, n_part, items)()
        order_by(cols)()
        torch.cuda.synchronize()
        p, v = part32[perm], ints[perm]
        want = torch.zeros_like(v)
        want[1:] = torch.where(p[1:] == p[:-1], v[:-1], torch.zeros_like(v[1:]))
        lines.append(f"check (i): along the sorted rows LAG is the left neighbour's cell, 0 at a partition's first row: "
                     f"{bool((outs[0][perm] == want).all())}")
    if "q" in a.case:  # checked with torch over the sort's own row list: one partition, so a difference of i64 prefix sums
        what, keys, _ = frame_cases["q"]
        _, cols, n_part, _ = cases[keys]
        window_frames(cols, n_part, [(hs.WIN_SUM, vi, 500, 500)])()
        order_by(cols)()
        torch.cuda.synchronize()
        prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(ints[perm].to(torch.int64), 0)])
        position = torch.arange(n, device="cuda")
        want = prefix[torch.clamp(position + 501, max=n)] - prefix[torch.clamp(position - 500, min=0)]
        ok = bool((outs[0][perm].to(torch.int64) == want).all()) and int(flags[0].item()) == 0
        lines.append(f"check (q): along the sorted rows SUM(INTEGER) over (500, 500) is the sum of the 1001 cells around the row: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
