"""What a date part costs as a GROUP BY key: SUM(l_quantity) grouped by a projected YEAR(l_shipdate) against the same sum
grouped by a stored INTEGER column holding the same years, over the synthetic lineitem, through HipExecutionEngine.

  (s)  SELECT l_year, SUM(l_quantity) ... GROUP BY l_year                    the stored column: 4 B key + 4 B value per row
  (y)  select(YEAR(l_shipdate) AS y, l_quantity).group_by(y).agg(SUM)        the projected part: the engine evaluates the
       projection (hs_eval: 8 B timestamp in, 8 B cell out), then groups by the evaluated column
  (p)  the projection of (y) alone, through hs_eval: rows in, one part out - the opcode's own kernel

Both queries take the same aggregation path behind the key column, so (y) - (s) is the cost of forming the part.  l_year is
made once, before the timing, from the engine's own YEAR (and checked against numpy's datetime64 on a sample).  Per repeat
every query runs once, in turn.  Clock: a HIP event pair on the launch stream around collect() / run().  Reported: median
(min - max) over --reps, the difference per row, and the instructions per row it implies at the kernel's measured rate.
Usage: python tools/bench_date_parts.py [--sf 10] [--reps 20] [--warmup 3] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from minispark_amd import hipspark as hs  # noqa: E402
from minispark_amd import synth  # noqa: E402
from minispark_amd.constants import ColumnType  # noqa: E402
from minispark_amd.dataframe import DataFrame  # noqa: E402
from minispark_amd.device import DCol  # noqa: E402
from minispark_amd.execution import HipExecutionEngine  # noqa: E402
from minispark_amd.io import BlockFile  # noqa: E402
from minispark_amd.sql import Col, Functions as F  # noqa: E402
from minispark_amd.table import DeviceTable  # noqa: E402


def word(op: int, sp: int, a: int = 0) -> int:
    return op | (sp << 8) | (a << 16)


def part_program(selector: int) -> hs.hs_program:
    p = hs.hs_program()
    for i, w in enumerate([word(hs.OP_LD, 0, 0), word(hs.OP_DATEPART, 1, selector), word(hs.OP_OUT, 1, 0)]):
        p.ins[i] = w
    p.n_ins = 3
    return p


def eval_part(dev, ship: DCol, selector: int, out: torch.Tensor) -> None:
    cols = (hs.hs_col * 1)(ship.as_hs())
    prog = part_program(selector)
    ptrs, kinds = (C.c_void_p * 1)(out.data_ptr()), (C.c_int32 * 1)(hs.I64)
    hs.check(dev.lib.hs_eval(dev.stream, cols, 1, C.byref(prog), None, ship.n, None, ptrs, kinds, 1, dev.flags.data_ptr()), "hs_eval")


def with_year_column(engine, table: DeviceTable, path: Path) -> DeviceTable:
    """The lineitem's columns plus l_year INTEGER = YEAR(l_shipdate), as a second resident table."""
    dev = engine.dev
    ship = table.columns[6]
    cells = dev.empty(ship.n, torch.int64)
    eval_part(dev, ship, 0, cells)
    year = cells.to(torch.int32)
    sample = slice(0, min(ship.n, 1 << 20))
    want = ship.data[sample].cpu().numpy().view("datetime64[us]").astype("datetime64[Y]").astype(np.int64) + 1970
    assert (year[sample].cpu().numpy() == want).all(), "YEAR differs from numpy's datetime64"
    schema = [*table.schema, ("l_year", ColumnType.INTEGER)]
    BlockFile(path, schema).write_rows([])  # header only
    out = DeviceTable(path, schema, list(table.block_rows), {}, ())
    out.global_blocks, out.total_blocks = list(table.global_blocks), table.total_blocks
    for i, col in table.columns.items():
        out.columns[i] = col
    out.columns[len(schema) - 1] = DCol(hs.I32, year, ship.n)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = synth.lineitem_rows(a.sf)
    lines = [f"tools/bench_date_parts.py --sf {a.sf:g} --reps {a.reps}   [{torch.cuda.get_device_name(0)}, torch {torch.__version__}]",
             f"rows={rows}; SUM(l_quantity) by year; median (min - max) ms over {a.reps} repeats, every query once per repeat"]
    with HipExecutionEngine(device=0, work_folder=Path(tempfile.mkdtemp(prefix="hipspark_dp_"))) as engine:
        folder = Path(tempfile.mkdtemp(prefix="hipspark_dp_t_"))
        plain = synth.make_lineitem(engine.dev, folder / "lineitem.bin", rows)
        engine.attach_device_table(folder / "lineitem.bin", plain)
        engine.attach_device_table(folder / "lineitem_y.bin", with_year_column(engine, plain, folder / "lineitem_y.bin"))
        qty, ship = Col("l_quantity"), Col("l_shipdate")

        def stored():
            return DataFrame(engine).table(str(folder / "lineitem_y.bin")).group_by(Col("l_year")).agg(F.sum(qty).alias("q"))

        def projected():
            return (DataFrame(engine).table(str(folder / "lineitem.bin")).select(F.year(ship).alias("y"), qty).group_by(Col("y"))
                    .agg(F.sum(qty).alias("q")))

        cells = engine.dev.empty(rows, torch.int64)
        runs = {"s": lambda: stored().collect(), "y": lambda: projected().collect(),
                "p": lambda: eval_part(engine.dev, plain.columns[6], 0, cells)}
        results = {}
        for name, run in runs.items():
            for _ in range(max(a.warmup, 3)):
                results[name] = run()
        times = {name: [] for name in runs}
        stream = torch.cuda.current_stream(engine.dev.device)
        for _ in range(a.reps):
            for name, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        for name, ts in times.items():
            lines.append(f"({name}) step {statistics.median(ts):8.3f} ms ({min(ts):.3f} - {max(ts):.3f})   "
                         f"spread (max - min) / median {(max(ts) - min(ts)) / statistics.median(ts):.4f}")
        med = {name: statistics.median(ts) for name, ts in times.items()}
        by_stored = {r["l_year"]: r["q"] for r in results["s"]}
        by_part = {r["y"]: r["q"] for r in results["y"]}
        lines.append(f"check: {len(by_part)} years, the two queries' sums equal: {by_stored == by_part}")
        extra_ns = (med["y"] - med["s"]) * 1e6 / rows
        lines.append(f"(y) - (s) = {med['y'] - med['s']:.3f} ms = {extra_ns:.4f} ns per row; (p) alone {med['p'] * 1e6 / rows:.4f} ns per row "
                     f"= {rows * 16 / (med['p'] * 1e-3) / 1e12:.2f} TB/s over its 16 B per row")
        # instructions per row the part can cost: at the rate (p) ran, the row's share of the card's vector issue slots
        props = torch.cuda.get_device_properties(0)
        ghz = getattr(props, "clock_rate", 2_400_000) / 1e6  # kHz where the build reports it, else the MI355X's 2.4 GHz peak
        slots_per_ns = props.multi_processor_count * 4 * 16 * ghz  # CUs x SIMDs x 16 lanes per cycle x GHz
        lines.append(f"(p): at most {med['p'] * 1e6 / rows * slots_per_ns:.0f} lane-instructions per row fit in its time "
                     f"({props.multi_processor_count} CUs x 4 SIMDs x 16 lanes per cycle at {ghz:.2f} GHz) - the kernel is bound by "
                     "its 16 B per row when that is more than the part's arithmetic needs")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
