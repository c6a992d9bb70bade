"""COUNT(DISTINCT) benchmark, HIP events on the launch stream, median and min - max of --reps runs after warm-up.

1. hs_mark_first on its sort path (mode 1) and its dense path (mode 2), next to hs_order_by without a limit over the same
   keys - the sort is shared, so that is the floor of the sort path:
     (a)-(e) one INTEGER column with 2^8, 2^16, 2^20, 2^22, 2^24 different values
     (f)     a (code byte, INTEGER) pair: 4 codes x 2^16 values
     (g)     a two-word key (TIMESTAMP, INTEGER), 2^20 different rows: sort path only
   MF_DENSE_BITS (hs_radix.hip) follows the largest of these at which the dense path is still the faster one.
2. End to end on the synthetic lineitem at every --sf:
     SELECT l_returnflag, COUNT(DISTINCT l_orderkey), SUM(l_quantity) FROM lineitem GROUP BY l_returnflag
   against the same query without the distinct item (collect() with the table resident).
All calls read a few words back between their steps, so their times include those host round trips.
Usage: python tools/bench_count_distinct.py [--rows 64M] [--reps 20] [--sf 1 10] [--out profiles/r14_count_distinct.txt]"""
from __future__ import annotations

import argparse
import ctypes as C
import socket
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402
from tools.bench_order_by import timed  # noqa: E402


def kernel_level(lib, n: int, reps: int, lines: list[str], flush) -> None:
    g = torch.Generator(device="cuda")
    g.manual_seed(14)
    stream = torch.cuda.current_stream().cuda_stream
    marks = torch.empty(n, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.hs_mark_first_ws_bytes(n, 2, 3)) + 256, dtype=torch.uint8, device="cuda")
    count = C.c_int64(0)
    col = lambda kind, t, fixed=-1: hs.hs_col(kind, fixed, t.data_ptr(), None, None)  # noqa: E731

    def values(bits):
        return torch.randint(0, 1 << bits, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)

    cases = []
    keep = []
    for tag, bits in zip("abcde", (8, 16, 20, 22, 24)):
        v = values(bits)
        keep.append(v)
        cases.append((tag, f"INTEGER, 2^{bits} values", [col(hs.I32, v)], True))
    codes = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
    lens = torch.ones(n, dtype=torch.uint8, device="cuda")
    coded = hs.hs_col(hs.STR, 1, codes.data_ptr(), lens.data_ptr(), None)
    cases.append(("f", "(code byte, INTEGER), 4 x 2^16", [coded, col(hs.I32, keep[1])], True))
    stamps = keep[2].to(torch.int64) * 1_000_003 + 1_700_000_000_000_000
    cases.append(("g", "(TIMESTAMP, INTEGER), 2^20 rows", [col(hs.I64, stamps), col(hs.I32, keep[2])], False))

    def mark_first(cols, mode):
        arr = (hs.hs_col * len(cols))(*cols)

        def run():
            hs.check(lib.hs_mark_first(stream, arr, len(cols), n, None, 0, mode, marks.data_ptr(), ws.data_ptr(), None),
                     "hs_mark_first")
        return run

    def order_by(cols):
        arr = (hs.hs_col * len(cols))(*cols)
        asc = (C.c_int32 * len(cols))(*[0] * len(cols))

        def run():
            hs.check(lib.hs_order_by(stream, arr, asc, len(cols), n, None, -1, perm.data_ptr(), C.byref(count), ws.data_ptr(),
                                     None), "hs_order_by")
        return run

    lines.append(f"1. hs_mark_first over {n} rows; median (min - max) ms, rows/s at the median; the marks of both modes are "
                 "compared cell by cell")
    for tag, what, cols, dense in cases:
        ms, lo, hi = timed(mark_first(cols, 1), reps)
        total = int(marks.sum().item())
        sort_marks = marks.clone()
        lines.append(f"({tag}) mode 1 sort   {what:32s} {ms:9.3f} ms ({lo:.3f} - {hi:.3f})   {n / ms / 1e6:8.2f} G rows/s   "
                     f"{total} marks")
        if dense:
            md, dlo, dhi = timed(mark_first(cols, 2), reps)
            same = bool(torch.equal(marks, sort_marks))
            verdict = "dense faster beyond the spread" if md + (dhi - dlo) < ms - (hi - lo) else "NOT faster beyond the spread"
            lines.append(f"({tag}) mode 2 dense  {what:32s} {md:9.3f} ms ({dlo:.3f} - {dhi:.3f})   {n / md / 1e6:8.2f} G rows/s   "
                         f"sort / dense {ms / md:.2f}   same marks: {same}   {verdict}")
            m0, lo0, hi0 = timed(mark_first(cols, 0), reps)
            lines.append(f"({tag}) mode 0 auto   {what:32s} {m0:9.3f} ms ({lo0:.3f} - {hi0:.3f})")
        mo, lo, hi = timed(order_by(cols), reps)
        lines.append(f"({tag}) hs_order_by   {what:32s} {mo:9.3f} ms ({lo:.3f} - {hi:.3f})   {n / mo / 1e6:8.2f} G rows/s   "
                     f"mode 1 / hs_order_by {ms / mo:.2f}")
        del sort_marks
        flush()


def end_to_end(sfs: list[float], reps: int, lines: list[str], flush) -> None:
    from minispark_amd import synth
    from minispark_amd.execution import HipExecutionEngine
    from minispark_amd.workloads import engine_api

    lines.append("2. SELECT l_returnflag, COUNT(DISTINCT l_orderkey), SUM(l_quantity) ... GROUP BY l_returnflag, collect() with the "
                 "table resident, against the same query without the distinct item")
    for sf in sfs:
        scratch = Path(tempfile.mkdtemp(prefix="hipspark_cd_"))
        with HipExecutionEngine(device=0, work_folder=scratch) as engine:
            rows = synth.lineitem_rows(sf)
            path = scratch / f"lineitem_sf{sf:g}.bin"
            engine.attach_device_table(path, synth.make_lineitem(engine.dev, path, rows, with_orderkey=True))
            api = engine_api(engine)
            C_, F = api.Col, api.F
            by_flag = lambda *aggs: api.DataFrame().table(str(path)).group_by(C_("l_returnflag")).agg(*aggs)  # noqa: E731
            with_count = by_flag(F.count_distinct(C_("l_orderkey")).alias("orders"), F.sum(C_("l_quantity")))
            without = by_flag(F.sum(C_("l_quantity")))
            got = {}
            mw, lo, hi = timed(lambda: got.__setitem__("rows", with_count.collect()), reps)
            mp, plo, phi = timed(lambda: without.collect(), reps)
            orders = {r["l_returnflag"]: r["orders"] for r in got["rows"]}
            lines.append(f"sf={sf:g} ({rows} rows) with COUNT(DISTINCT)    {mw:9.3f} ms ({lo:.3f} - {hi:.3f})   "
                         f"{rows / mw / 1e6:8.2f} G rows/s   {orders}")
            lines.append(f"sf={sf:g} ({rows} rows) without                 {mp:9.3f} ms ({plo:.3f} - {phi:.3f})   "
                         f"{rows / mp / 1e6:8.2f} G rows/s   ratio {mw / mp:.1f}")
        flush()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=64 * 2**20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sf", type=float, nargs="*", default=[1.0, 10.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(a.rows)
    lib = hs.load_library()
    lines = [f"tools/bench_count_distinct.py --rows {n} --reps {a.reps} --sf {' '.join(f'{s:g}' for s in a.sf)}   "
             f"[{torch.cuda.get_device_name(0)}, host {socket.gethostname()}, torch {torch.__version__}]",
             "events on the launch stream around the whole call, host round trips included"]
    shown = [0]

    def flush() -> None:  # every finished case at once: a later failure loses nothing
        print("\n".join(lines[shown[0]:]), flush=True)
        shown[0] = len(lines)
        if a.out:
            Path(a.out).write_text("\n".join(lines) + "\n")

    kernel_level(lib, n, a.reps, lines, flush)
    torch.cuda.empty_cache()
    end_to_end(a.sf, a.reps, lines, flush)
    flush()


if __name__ == "__main__":
    main()
